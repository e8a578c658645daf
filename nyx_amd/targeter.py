"""The differential-correction targeter: `Targeter::try_achieve_fd` (md/opti/targeter.rs with raphson_finite_diff.rs), the branch
without a finite burn, for a whole batch.

A Newton-Raphson differential corrector: it varies components of a state at a correction epoch until chosen parameters of the
propagated state reach desired values at an achievement epoch.  `target_definition` is the HOST DEFINITION, scalar float64 with one
rounding per operation and every sum taken left to right from its first term; `csrc/target_dev.h` restates it operation for operation
for the device, `include/nyx_hip_target.h` states it in words.  The propagation is injected (`propagate_fn`): the CPU oracle in the
CPU tests, `GpuContext.propagate_until_epoch` as the reference of the fused device loop (`GpuContext.target`).

Kept as the reference writes it: the clamp is ONE if / else-if chain per variable and acts ON THE STEP, not on the total -
|d| > |max_step| gives |max_step| sign(d), else d > max_value gives max_value, else d < min_value gives min_value - and a run that
falls out of the loop has taken its last step (TOO_MANY_ITERATIONS).

TWO DEPARTURES.  (1) THE SOLVE.  The reference forms a pseudo-inverse through nalgebra's `try_inverse`.  Here, with O objectives and V
variables, O < V solves (J J^T) y = err and takes d = J^T y (the minimum-norm step), otherwise (J^T J) d = J^T err (least squares),
both by an UNPIVOTED CHOLESKY factorisation written out operation for operation.  It is the same step; a Gram matrix needs no
pivoting - hence no dynamically indexed registers on the device - and no explicit inverse; a pivot that is not finite or not > 0
gives SINGULAR.  (2) THE VNC FRAME IS THAT OF xi_start FOR THE WHOLE RUN.  The reference applies every perturbation and step in the frame of
the current xi, sums the steps, and reports the corrected state with that sum applied in the frame of xi_start; the frame turns with
the velocity, and for the 3 km/s correction of tests/target_cases.py `vnc` the reported correction, flown again, missed Eccentricity 0.4
by 0.0723 (tolerance 1e-5).  With one frame the total is the sum of the steps and `corrected` the state they led to.

Which test wins: EPHEM_RANGE (the achievement epoch lies outside the objective target's chain), PROP_FAILED (one of the run's 1 + V
rows, or its leg to the correction epoch, ended with a non-zero propagation status), NOT_FINITE (an achieved value or a Jacobian
entry is NaN or +-inf: a B-plane objective on an ellipse, the reference's NotHyperbolic), CONVERGED, INEFFECTIVE, SINGULAR,
TOO_MANY_ITERATIONS.  A run that ends keeps its last total, err and achieved state; with EPHEM_RANGE and PROP_FAILED the errors are NaN.
"""
from __future__ import annotations

import dataclasses
import enum
import math
from typing import List, Optional, Sequence

import numpy as np

from . import _abi, frames
from .frames import FrameParameter

MAX_VARS = 6
MAX_OBJS = 6
MAX_ITERATIONS = 1000


class TargetStatus(enum.IntEnum):
    """enum nyx_hip_target_status (include/nyx_hip_target.h): never renumber."""

    OK_CONVERGED = 0
    TOO_MANY_ITERATIONS = 1
    INEFFECTIVE = 2
    SINGULAR = 3
    NOT_FINITE = 4
    PROP_FAILED = 5
    EPHEM_RANGE = 6


class Vary(enum.IntEnum):
    """The reference's `Vary`, the impulsive components only: the index of the state component."""

    PositionX = 0
    PositionY = 1
    PositionZ = 2
    VelocityX = 3
    VelocityY = 4
    VelocityZ = 5


@dataclasses.dataclass
class Variable:
    """The reference's `Variable` with its defaults."""

    component: Vary
    perturbation: float = 1e-4
    init_guess: float = 0.0
    max_step: float = 0.2
    max_value: float = 5.0
    min_value: float = -5.0

    def check(self, j: int = 0):
        """What `check_target` (csrc/target_args.h) refuses of a variable, with its words."""
        name = "target_batch"
        if not 0 <= int(self.component) < 6:
            raise ValueError(f"{name}: var_component[{j}] = {int(self.component)} is not a nyx_hip_target_vary")
        if not (math.isfinite(self.perturbation) and self.perturbation != 0.0):
            raise ValueError(f"{name}: var_perturbation[{j}] must be finite and not zero")
        if not math.isfinite(self.init_guess):
            raise ValueError(f"{name}: var_init_guess[{j}] must be finite")
        if not self.max_step >= 0.0:
            raise ValueError(f"{name}: var_max_step[{j}] must be >= 0")
        if not self.max_value >= 0.0:
            raise ValueError(f"{name}: var_max_value[{j}] must be >= 0")
        if not self.min_value <= self.max_value:
            raise ValueError(f"{name}: var_min_value[{j}] must be <= var_max_value[{j}]")


@dataclasses.dataclass
class Objective:
    """The reference's `Objective`."""

    parameter: FrameParameter
    desired_value: float
    tolerance: float
    multiplicative_factor: float = 1.0
    additive_factor: float = 0.0

    @classmethod
    def within_tolerance(cls, parameter, desired_value: float, tolerance: float) -> "Objective":
        return cls(frames.frame_param(parameter), float(desired_value), float(tolerance))

    def check(self, o: int = 0):
        name = "target_batch"
        frames.frame_param(self.parameter)
        if not (math.isfinite(self.tolerance) and self.tolerance >= 0.0):
            raise ValueError(f"{name}: obj_tolerance[{o}] must be finite and >= 0")
        if not (math.isfinite(self.desired_value) and math.isfinite(self.multiplicative_factor) and math.isfinite(self.additive_factor)):
            raise ValueError(f"{name}: obj_desired[{o}], obj_mult[{o}] and obj_add[{o}] must be finite")


@dataclasses.dataclass
class BPlaneTarget:
    """The reference's `BPlaneTarget` without the linearised time of flight (`BLTOF` has no code here)."""

    b_t_km: float
    b_r_km: float
    tol_b_t_km: float = 1.0
    tol_b_r_km: float = 1.0

    @classmethod
    def from_bt_br(cls, b_t_km: float, b_r_km: float, tol_km: float = 1.0) -> "BPlaneTarget":
        return cls(float(b_t_km), float(b_r_km), float(tol_km), float(tol_km))

    def to_objectives(self) -> List[Objective]:
        return [Objective.within_tolerance(FrameParameter.BdotR, self.b_r_km, self.tol_b_r_km),
                Objective.within_tolerance(FrameParameter.BdotT, self.b_t_km, self.tol_b_t_km)]


def check_problem(variables: Sequence[Variable], objectives: Sequence[Objective], correction_frame, iterations: int):
    """The refusals of `check_target` that can be told on the host, in its order and with its words; returns the frame code."""
    name = "target_batch"
    if not 1 <= len(variables) <= MAX_VARS:
        raise ValueError(f"{name}: n_vars = {len(variables)}, 1 .. {MAX_VARS} variables")
    if not 1 <= len(objectives) <= MAX_OBJS:
        raise ValueError(f"{name}: n_objs = {len(objectives)}, 1 .. {MAX_OBJS} objectives")
    if not 0 <= int(iterations) <= MAX_ITERATIONS:
        raise ValueError(f"{name}: iterations = {int(iterations)}, 0 .. {MAX_ITERATIONS}")
    if correction_frame not in (None, "VNC"):
        raise ValueError(f"{name}: correction_frame = {correction_frame!r}, None (inertial) or 'VNC'")
    for j, v in enumerate(variables):
        v.check(j)
        if correction_frame == "VNC" and int(v.component) < 3:
            raise ValueError(f"{name}: var_component[{j}] is a position: a correction frame takes velocity variables only")
    for o, obj in enumerate(objectives):
        obj.check(o)
    return _abi.FRAME_VNC if correction_frame == "VNC" else _abi.FRAME_INERTIAL


# ---- the scalar pieces: csrc/target_dev.h restates each under the same name

def _c6(variables, val) -> List[float]:
    """tgt_c6: c6 = 0, then c6[component_j] = c6[component_j] + val[j] in the order of the variables."""
    c6 = [0.0] * 6
    for j, v in enumerate(variables):
        c6[int(v.component)] = c6[int(v.component)] + float(val[j])
    return c6


def _apply(vnc: bool, frm, c6, x) -> List[float]:
    """tgt_apply: x (+) c6 in the inertial frame, or in the VNC frame of the state `frm`."""
    x = [float(t) for t in x]
    if not vnc:
        return [x[k] + c6[k] for k in range(6)]
    f = [float(t) for t in frm]
    h0, h1, h2 = f[1] * f[5] - f[2] * f[4], f[2] * f[3] - f[0] * f[5], f[0] * f[4] - f[1] * f[3]
    hn = _sqrt((h0 * h0 + h1 * h1) + h2 * h2)
    vn = _sqrt((f[3] * f[3] + f[4] * f[4]) + f[5] * f[5])
    e00, e01, e02 = _div(f[3], vn), _div(f[4], vn), _div(f[5], vn)
    e10, e11, e12 = _div(h0, hn), _div(h1, hn), _div(h2, hn)
    e20, e21, e22 = e01 * e12 - e02 * e11, e02 * e10 - e00 * e12, e00 * e11 - e01 * e10
    x[3] = x[3] + ((e00 * c6[3] + e10 * c6[4]) + e20 * c6[5])
    x[4] = x[4] + ((e01 * c6[3] + e11 * c6[4]) + e21 * c6[5])
    x[5] = x[5] + ((e02 * c6[3] + e12 * c6[4]) + e22 * c6[5])
    return x


def _sqrt(x: float) -> float:
    return math.sqrt(x) if x >= 0.0 else math.nan   # (a NaN or a negative argument: NaN, as in C)


def _div(a: float, b: float) -> float:
    if b == 0.0:   # IEEE: x / 0 = +-inf, 0 / 0 = NaN
        if a == 0.0 or a != a:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def start_states(variables, vnc: bool, frm, xi) -> List[List[float]]:
    """tgt_start_state for k = 0 .. V: the nominal and the perturbed states of a round; `frm` is xi_start, whose VNC frame is THE
    correction frame of the run."""
    out = [[float(t) for t in xi]]
    for v in variables:
        only = [0.0] * 6
        only[int(v.component)] = only[int(v.component)] + float(v.perturbation)
        out.append(_apply(vnc, frm, only, xi))
    return out


def cholesky_solve(G, b, m: int):
    """The unpivoted Cholesky solve of the m x m system G x = b (the lower triangle of G is read), operation for operation as
    tgt_step writes it; None where a pivot is not finite or not > 0."""
    L = [[0.0] * m for _ in range(m)]
    for i in range(m):
        for j in range(i + 1):
            s = G[i][j]
            for k in range(j):
                s = s - L[i][k] * L[j][k]
            if i == j:
                if not (s > 0.0) or not math.isfinite(s):
                    return None
                L[i][i] = math.sqrt(s)
            else:
                L[i][j] = _div(s, L[j][j])
    y = [0.0] * m
    for i in range(m):
        s = b[i]
        for k in range(i):
            s = s - L[i][k] * y[k]
        y[i] = _div(s, L[i][i])
    x = [0.0] * m
    for i in range(m - 1, -1, -1):
        s = y[i]
        for k in range(i + 1, m):
            s = s - L[k][i] * x[k]
        x[i] = _div(s, L[i][i])
    return x


def newton_step(variables, objectives, vals, prev: float):
    """The middle of tgt_step for one run: `vals[k][i]` the value of objective i at final state k.  Returns (status or None, err, nrm,
    delta): status None means the step `delta` (clamped) is to be taken."""
    V, O = len(variables), len(objectives)
    val0 = [float(vals[0][i]) for i in range(O)]
    J = [[_div(float(vals[1 + j][i]) - val0[i], float(variables[j].perturbation)) for j in range(V)] for i in range(O)]
    not_finite = any(not math.isfinite(v) for v in val0) or any(not math.isfinite(J[i][j]) for i in range(O) for j in range(V))
    err = [float(o.multiplicative_factor) * (float(o.desired_value) - val0[i]) + float(o.additive_factor) for i, o in enumerate(objectives)]
    if not_finite:
        return TargetStatus.NOT_FINITE, err, prev, None
    if all(abs(err[i]) <= float(objectives[i].tolerance) for i in range(O)):
        return TargetStatus.OK_CONVERGED, err, prev, None
    ss = err[0] * err[0]
    for i in range(1, O):
        ss = ss + err[i] * err[i]
    nrm = math.sqrt(ss)
    if abs(nrm - prev) < 1e-10:
        return TargetStatus.INEFFECTIVE, err, prev, None
    if O < V:
        G = [[0.0] * O for _ in range(O)]
        for a in range(O):
            for c in range(a + 1):
                g = J[a][0] * J[c][0]
                for j in range(1, V):
                    g = g + J[a][j] * J[c][j]
                G[a][c] = g
        yv = cholesky_solve(G, err, O)
        if yv is None:
            return TargetStatus.SINGULAR, err, nrm, None
        delta = []
        for j in range(V):
            d = J[0][j] * yv[0]
            for a in range(1, O):
                d = d + J[a][j] * yv[a]
            delta.append(d)
    else:
        G = [[0.0] * V for _ in range(V)]
        b = []
        for a in range(V):
            r = J[0][a] * err[0]
            for i in range(1, O):
                r = r + J[i][a] * err[i]
            b.append(r)
            for c in range(a + 1):
                g = J[0][a] * J[0][c]
                for i in range(1, O):
                    g = g + J[i][a] * J[i][c]
                G[a][c] = g
        delta = cholesky_solve(G, b, V)
        if delta is None:
            return TargetStatus.SINGULAR, err, nrm, None
    for j, v in enumerate(variables):
        ms, d = abs(float(v.max_step)), delta[j]
        if abs(d) > ms:
            d = ms if d > 0.0 else -ms
        elif d > float(v.max_value):
            d = float(v.max_value)
        elif d < float(v.min_value):
            d = float(v.min_value)
        delta[j] = d
    return None, err, nrm, delta


class TargeterSolutions:
    """What a targeter run of a batch returns: per run `status` (TargetStatus), `iterations`, `correction[V, n]` (the total),
    `achieved_errors[O, n]`, the `corrected` state at the correction epoch and the `achieved` state (the nominal's last final state,
    about the context's centre) as StateBatches; `iterations_run` propagation rounds were run."""

    def __init__(self, variables, objectives, status, iterations, correction, achieved_errors, corrected, achieved, iterations_run: int):
        self.variables, self.objectives = list(variables), list(objectives)
        self.status, self.iterations = np.asarray(status, dtype=np.int32), np.asarray(iterations, dtype=np.int32)
        self.correction, self.achieved_errors = np.asarray(correction, dtype=np.float64), np.asarray(achieved_errors, dtype=np.float64)
        self.corrected, self.achieved = corrected, achieved
        self.iterations_run = int(iterations_run)

    @property
    def n(self) -> int:
        return len(self.status)

    @property
    def converged(self) -> np.ndarray:
        return self.status == int(TargetStatus.OK_CONVERGED)

    @property
    def converged_fraction(self) -> float:
        return float(self.converged.mean()) if self.n else 0.0

    def delta_v_norm(self) -> np.ndarray:
        """|dv| of every run: the Euclidean norm of the velocity components of its correction (in the correction frame)."""
        rows = [j for j, v in enumerate(self.variables) if int(v.component) >= 3]
        return np.sqrt((self.correction[rows] ** 2).sum(axis=0)) if rows else np.zeros(self.n)


def _rows_batch(template: _abi.StateBatch, index, rv, epoch_ns: int) -> _abi.StateBatch:
    """The runs `index` of `template` (their Cr, Cd, masses and areas) with the states `rv` at `epoch_ns`, the step left to the
    context's initial step."""
    b = template.take(index)
    b.set_rv(np.asarray(rv, dtype=np.float64).reshape(len(index), 6))
    b.epoch_ns[:] = int(epoch_ns)
    b.step_ns[:] = 0
    if b.stm is not None:
        b.stm = None
    return b


def target_definition(propagate_fn, batch: _abi.StateBatch, variables: Sequence[Variable], objectives: Sequence[Objective], correction_epoch_ns: int,
                      achievement_epoch_ns: int, mu: float, objective_target=None, almanac=None, central=None, correction_frame=None,
                      iterations: int = 100) -> TargeterSolutions:
    """`try_achieve_fd` for every run of `batch`.  `propagate_fn(batch, end_epoch_ns) -> (batch, stats)` propagates a StateBatch to
    an epoch (stats.status per row).  `mu` is the gravitational parameter the objectives are evaluated with; with `objective_target`
    (a Frame of `almanac`, whose centre is `central`) every final state is translated to it first, exactly as `frames.to_frame`
    does, and its own mu is used.  The rounds are taken for all runs still active at once: one call of `propagate_fn` per round."""
    check_problem(variables, objectives, correction_frame, iterations)
    vnc = correction_frame == "VNC"
    variables, objectives = list(variables), list(objectives)
    V, O, n = len(variables), len(objectives), batch.n
    if objective_target is not None:
        frames.check_target(objective_target, almanac, central)
        mu = float(objective_target.mu_km3_s2)
    mu = float(mu)
    if not (math.isfinite(mu) and mu > 0.0):
        raise ValueError("target_batch: mu_km3_s2 must be finite and > 0")
    status = np.full(n, -1, dtype=np.int32)
    its = np.zeros(n, dtype=np.int32)
    correction, errors = np.zeros((V, n)), np.full((O, n), np.nan)
    corrected, achieved = batch.copy(), batch.copy()
    corrected.stm = achieved.stm = None
    if n == 0:
        return TargeterSolutions(variables, objectives, status, its, correction, errors, corrected, achieved, 0)
    # start-up: the leg to the correction epoch, the initial guesses
    start, st0 = propagate_fn(batch, int(correction_epoch_ns))
    leg_failed = np.asarray(st0.status) != 0
    xs = start.rv()
    guess = [float(v.init_guess) for v in variables]
    xi = [_apply(vnc, xs[i], _c6(variables, guess), xs[i]) for i in range(n)]
    total = [list(guess) for _ in range(n)]
    prev = [math.inf] * n
    # the objective target at the achievement epoch: one state for the batch
    ephem_bad, body = False, None
    if objective_target is not None and frames.body_chain(objective_target.naif_id, almanac, central):
        r, v = frames.body_state(objective_target.naif_id, np.asarray([int(achievement_epoch_ns)], dtype=np.int64), almanac, central)
        body = np.concatenate([r[0], v[0]])
        ephem_bad = not np.isfinite(body).all()
    for f in _abi.F64_FIELDS[6:]:
        getattr(corrected, f)[:] = getattr(start, f)
    corrected.epoch_ns[:] = int(correction_epoch_ns)
    active = list(range(n))
    rounds = 0
    for it in range(int(iterations) + 1):
        rows = np.array([start_states(variables, vnc, xs[i], xi[i]) for i in active])              # [n_active, 1 + V, 6]
        index = np.tile(np.asarray(active, dtype=np.int64), 1 + V)                            # row k n_active + a
        work = _rows_batch(start, index, rows.transpose(1, 0, 2).reshape(-1, 6), correction_epoch_ns)
        final, fst = propagate_fn(work, int(achievement_epoch_ns))
        rounds = it + 1
        na = len(active)
        xf = final.rv().reshape(1 + V, na, 6)
        pst = np.asarray(fst.status).reshape(1 + V, na)
        about = xf - body if body is not None else xf
        with np.errstate(all="ignore"):
            vals = np.array([[frames.state_frame_value(o.parameter, about[k], mu) for o in objectives] for k in range(1 + V)])   # [1 + V, O, n_active]
        still = []
        for a, i in enumerate(active):
            stt, err = None, None
            if ephem_bad:
                stt = TargetStatus.EPHEM_RANGE
            elif leg_failed[i] or (pst[:, a] != 0).any():
                stt = TargetStatus.PROP_FAILED
            else:
                stt, err, prev[i], delta = newton_step(variables, objectives, vals[:, :, a], prev[i])
                if stt is None:
                    xi[i] = _apply(vnc, xs[i], _c6(variables, delta), xi[i])
                    total[i] = [total[i][j] + delta[j] for j in range(V)]
                    if it >= int(iterations):
                        stt = TargetStatus.TOO_MANY_ITERATIONS
            if stt is None:
                still.append(i)
                continue
            status[i], its[i] = int(stt), it
            correction[:, i] = total[i]
            if err is not None:
                errors[:, i] = err
            xc = _apply(vnc, xs[i], _c6(variables, total[i]), xs[i])
            for c, f in enumerate(_abi.F64_FIELDS[:6]):
                getattr(corrected, f)[i] = xc[c]
                getattr(achieved, f)[i] = xf[0, a, c]
            for f in _abi.F64_FIELDS[6:]:
                getattr(achieved, f)[i] = getattr(final, f)[a]
            achieved.epoch_ns[i] = final.epoch_ns[a]
        active = still
        if not active:
            break
    return TargeterSolutions(variables, objectives, status, its, correction, errors, corrected, achieved, rounds)


class Targeter:
    """The reference's `Targeter`: variables, objectives, an optional correction frame ("VNC") and objective frame, the iteration
    limit.  `try_achieve_from` runs the fused device loop of a GpuContext for a whole batch (`GpuContext.target`)."""

    def __init__(self, ctx, variables: Sequence[Variable], objectives: Sequence[Objective], objective_frame=None, correction_frame=None,
                 iterations: int = 100):
        self.ctx = ctx
        self.variables, self.objectives = list(variables), list(objectives)
        self.objective_frame, self.correction_frame, self.iterations = objective_frame, correction_frame, int(iterations)
        check_problem(self.variables, self.objectives, self.correction_frame, self.iterations)

    @classmethod
    def new(cls, ctx, variables, objectives) -> "Targeter":
        return cls(ctx, variables, objectives)

    @classmethod
    def in_frame(cls, ctx, variables, objectives, objective_frame) -> "Targeter":
        return cls(ctx, variables, objectives, objective_frame=objective_frame)

    @classmethod
    def vnc_with_components(cls, ctx, variables, objectives) -> "Targeter":
        return cls(ctx, variables, objectives, correction_frame="VNC")

    @classmethod
    def delta_v(cls, ctx, objectives) -> "Targeter":
        return cls(ctx, [Variable(Vary.VelocityX), Variable(Vary.VelocityY), Variable(Vary.VelocityZ)], objectives)

    @classmethod
    def delta_r(cls, ctx, objectives) -> "Targeter":
        return cls(ctx, [Variable(Vary.PositionX), Variable(Vary.PositionY), Variable(Vary.PositionZ)], objectives)

    @classmethod
    def vnc(cls, ctx, objectives) -> "Targeter":
        return cls(ctx, [Variable(Vary.VelocityX), Variable(Vary.VelocityY), Variable(Vary.VelocityZ)], objectives, correction_frame="VNC")

    def try_achieve_from(self, batch: _abi.StateBatch, correction_epoch_ns: int, achievement_epoch_ns: int) -> TargeterSolutions:
        return self.ctx.target(batch, self.variables, self.objectives, correction_epoch_ns, achievement_epoch_ns, objective_frame=self.objective_frame,
                               correction_frame=self.correction_frame, iterations=self.iterations)
