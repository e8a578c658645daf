"""Lambert transfers: Izzo's solver for one problem, a batch, and a departure x arrival grid (a porkchop).

Host-side DEFINITION of what csrc/lambert_dev.h computes on the device (include/nyx_hip_lambert.h is the contract).  The method is
D. Izzo, "Revisiting Lambert's problem" (2014), as the reference's `tools/lambert/izzo.rs` arranges it (`find_xy`, `initial_guess`,
`compute_t_min`, `halley`, `householder`, `reconstruct`), restated in scalar float64 with one rounding per operation and sums of three
formed as ((a0 + a1) + a2).  FOUR DEPARTURES from the reference, each for a measured reason:

1.  The orbit normal is the NATURAL one, ih = (i1 x i2) / |i1 x i2|, never flipped.  The reference flips ih to +z where (r1 x r2).z < 0
    without negating lambda or reversing the tangents (which lamberthub, the code it was adapted from, does): for r1 = (8000, 0, 0) km,
    r2 = (0, -8000, 0) km, 3600 s, mu = 398600.433 every one of its ways delivers a velocity that, flown, arrives 16 000 km from r2;
    with the natural normal all arrive within 3.2e-7 km.  SHORT is lambda = +sqrt(1 - c / s) with t_k = ih x i_k, LONG is lambda < 0 with
    t_k = i_k x ih; AUTO is the reference's rule as written (dnu = atan2(r2.y, r2.x) - atan2(r1.y, r1.x), + 2 pi if negative, LONG where
    dnu > pi: prograde about +z).  Where (r1 x r2).z > 0 this is the reference operation for operation, elsewhere it is lamberthub's rule.
2.  The series of the time equation is used for m == 0 and x > 0 and 0.6 < x x < 1.4.  The reference tests x x alone, which admits
    negative x: there the argument of `hyp2f1b` reaches 1.4 (the function returns +inf from 1 on, and just below 1 it needs tens of
    thousands of terms: 59 447 measured).  For x > 0 the argument stays within 0.4 in magnitude and at most 43 terms are needed;
    `hyp2f1b` stops when the sum no longer changes or after SERIES_MAX = 64 terms.
3.  The way applies to multi-revolution requests too, and `high_path` chooses the other of the two solutions (the reference's public
    entry pins the low path and the prograde way; its `find_xy(..., m, low_path)` takes both).
4.  The closed form of the time equation is evaluated without its cancellations.  The reference writes psi = acos(x y + lambda (1 - x x))
    and T = ((psi + m pi) / sqrt|1 - x x| - x + lambda y) / (1 - x x).  As lambda -> +-1 (r1 and r2 close together, or a transfer of nearly
    whole revolutions) psi -> 0, where half an ulp of the acos ARGUMENT is 1.1e-16 / sin(psi) in psi, and x - lambda y cancels.  On an
    Earth -> Moon grid about the Sun (lambda = 0.97, psi = 0.025) the definition so written moved its own root by 3.2e-13 when the start
    of its last Householder step was moved by two ulp: 53 times the K eps (|T / T'| + |x|) a solver of this order owes, and the device
    differed from it by 25 times that.  Here psi comes from its sine AND cosine, sin psi = eta sqrt(1 - x x), by atan2 (Izzo's eq. 17 with
    "the appropriate inverse function"; the reference itself takes sinh psi on a hyperbola), and where lambda x > 0 the two differences
    are formed from their products: eta = y - lambda x = (1 - lambda^2) / (y + lambda x) and
    x - lambda y = (1 - lambda^2)(x^2 (1 + lambda^2) - lambda^2) / (x + lambda y).  The same experiment then moves the root by 0.1 of that
    bound.  T is the same function.

Kept as written: Halley's iteration in `compute_t_min` evaluates the derivatives with T frozen at its first value (lamberthub and
poliastro do the same); it only moves the feasibility edge of a multi-revolution request.

Every problem has a status (LambertStatus); every value of a problem whose status is not OK is NaN.
"""
from __future__ import annotations

import enum
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import chains
from .chains import MAX_CHAIN, body_chain, cheby_state  # noqa: F401  (re-exported)
from .groundtrack import _TO_DEG, _ns_to_seconds


class TransferKind(enum.IntEnum):
    """enum nyx_hip_lambert_way: never renumber.  Revolutions are a separate argument (`n_revs`, `high_path`)."""

    Auto = 0
    ShortWay = 1
    LongWay = 2


class LambertStatus(enum.IntEnum):
    """enum nyx_hip_lambert_status: never renumber."""

    OK = 0
    BAD_INPUT = 1      # a non-finite component, |r1| == 0, |r2| == 0 or tof_s <= 0
    DEGENERATE = 2     # c == 0, or |i1 x i2| == 0 (the plane is undefined at 0 and pi)
    NOT_FEASIBLE = 3   # n_revs > m_max
    TOO_CLOSE = 4      # a denominator below 1e-14 in Halley or Householder
    MAX_ITER = 5       # iteration limit reached
    EPHEM_RANGE = 6    # grid only: an epoch outside a chain's segments


class LambertParameter(enum.IntEnum):
    """enum nyx_hip_lambert_param: never renumber."""

    V1X = 0
    V1Y = 1
    V1Z = 2
    V2X = 3
    V2Y = 4
    V2Z = 5
    X = 6                  # Izzo's variable
    Iterations = 7         # Householder steps taken, as a double
    TofS = 8
    TransferAngleDeg = 9
    C3 = 10                # |w|^2, w = v_init - v_body1
    VinfDep = 11           # |w|
    DlaDeg = 12            # asin(w.z / |w|)
    RlaDeg = 13            # atan2(w.y, w.x)
    VinfArr = 14           # |v_body2 - v_final|
    DvTotal = 15           # VinfDep + VinfArr


MAX_PARAMS = 8
SERIES_MAX = 64
MAX_REVS = 255
MAX_ITER_MOST = 1000
TOL_MIN, TOL_MAX = 1e-13, 1e-2
DEFAULT_TOL, DEFAULT_MAX_ITER = 1e-4, 1000
_PI = 3.14159265358979323846
_LN2 = 0.6931471805599453
_TWO_THIRDS = 2.0 / 3.0
_FOUR_THIRDS = 4.0 / 3.0
_NAN = float("nan")


def lambert_param(param) -> LambertParameter:
    if isinstance(param, LambertParameter):
        return param
    if isinstance(param, (int, np.integer)) and not isinstance(param, (bool, enum.Enum)):
        return LambertParameter(int(param))
    raise TypeError(f"{param!r} is not a LambertParameter")


def check_solver(way, n_revs: int, high_path, tol: float, max_iter: int):
    """What `check_lambert_query` (csrc/lambert_args.h) refuses of the solver's settings, on the host: ValueError."""
    way = TransferKind(int(way))
    if not 0 <= int(n_revs) <= MAX_REVS:
        raise ValueError(f"lambert: n_revs = {n_revs}, 0 .. {MAX_REVS}")
    if int(high_path) not in (0, 1):
        raise ValueError(f"lambert: high_path = {high_path}, 0 or 1")
    if not TOL_MIN <= float(tol) <= TOL_MAX:
        raise ValueError(f"lambert: tol = {tol}, {TOL_MIN} .. {TOL_MAX}")
    if not 1 <= int(max_iter) <= MAX_ITER_MOST:
        raise ValueError(f"lambert: max_iter = {max_iter}, 1 .. {MAX_ITER_MOST}")
    return way, int(n_revs), int(high_path), float(tol), int(max_iter)


class _Margin:
    """The smallest relative distance of a branch-deciding comparison from equality (`decision_margin`)."""

    def __init__(self):
        self.least = math.inf

    def cmp(self, a: float, b: float):
        scale = max(abs(a), abs(b))
        if math.isfinite(scale) and scale > 0.0:
            self.least = min(self.least, abs(a - b) / scale)
        elif scale == 0.0:
            self.least = 0.0


def _div(a: float, b: float) -> float:
    """IEEE division (Python raises where the device returns an infinity or a NaN)."""
    if b != 0.0:
        return a / b
    if a != a or a == 0.0:
        return _NAN
    return math.copysign(math.inf, a) * math.copysign(1.0, b)


def _sqrt(a: float) -> float:
    return math.sqrt(a) if a >= 0.0 else _NAN


class _Stop(Exception):
    def __init__(self, status):
        self.status = status


def _y(x, ll):
    return _sqrt(1.0 - (ll * ll) * (1.0 - x * x))


def hyp2f1b(x: float):
    """2F1(3, 1; 5/2; x) by its series: (value, terms added, whether the cap ended it)."""
    if x >= 1.0:
        return math.inf, 0, False
    res, term, ii = 1.0, 1.0, 0.0
    for k in range(SERIES_MAX):
        term = term * ((3.0 + ii) * (1.0 + ii) / (2.5 + ii) * x / (ii + 1.0))
        old = res
        res = res + term
        if res == old:
            return res, k + 1, False
        ii = ii + 1.0
    return res, SERIES_MAX, True


def in_series_window(x: float, m: int) -> bool:
    return m == 0 and x > 0.0 and 0.6 < x * x < 1.4


def _eta(x, y, ll):
    """eta = y - lam x.  Where lam x > 0 the difference cancels (y -> |lam x| as lam -> +-1): (y - lam x)(y + lam x) = 1 - lam^2."""
    if ll * x > 0.0:
        return (1.0 - ll * ll) / (y + ll * x)
    return y - ll * x


def _x_minus_lam_y(x, y, ll):
    """x - lam y.  Where lam x > 0 the difference cancels: (x - lam y)(x + lam y) = (1 - lam^2)(x^2 (1 + lam^2) - lam^2)."""
    if ll * x > 0.0:
        l2 = ll * ll
        return ((1.0 - l2) * ((x * x) * (1.0 + l2) - l2)) / (x + ll * y)
    return x - ll * y


def _psi(x, y, ll, eta):
    """Izzo's auxiliary angle: sinh psi = eta sqrt(x^2 - 1) on a hyperbola; on an ellipse sin psi = eta sqrt(1 - x^2) AND
    cos psi = x y + lam (1 - x^2), both (psi in [0, pi]: eta >= 0)."""
    if x > 1.0:
        return math.asinh(eta * _sqrt(x * x - 1.0))
    if x < 1.0:
        om = 1.0 - x * x
        return math.atan2(eta * _sqrt(om), x * y + ll * om)
    return 0.0


def time_of_flight(x, y, ll, m, mg: Optional[_Margin] = None):
    """Izzo's non-dimensional time T(x) for `m` revolutions (the reference's `tof_equation_y` with t0 = 0), its two differences formed
    without cancellation (departure 4 of the module's docstring)."""
    if mg is not None and m == 0:
        mg.cmp(x, 0.0)
        mg.cmp(x * x, 0.6)
        mg.cmp(x * x, 1.4)
    eta = _eta(x, y, ll)
    if in_series_window(x, m):
        s1 = ((1.0 - ll) - x * eta) * 0.5
        q = _FOUR_THIRDS * hyp2f1b(s1)[0]
        return (((eta * eta) * eta) * q + (4.0 * ll) * eta) * 0.5
    psi = _psi(x, y, ll, eta)
    den = 1.0 - x * x
    return _div(_div(psi + float(m) * _PI, _sqrt(abs(den))) - _x_minus_lam_y(x, y, ll), den)


def _derivs(x, y, t, ll):
    l2 = ll * ll
    l3 = l2 * ll
    l5 = (l2 * l2) * ll
    y2 = y * y
    y3 = y2 * y
    y5 = (y2 * y2) * y
    om = 1.0 - x * x
    d1 = _div(((3.0 * t) * x - 2.0) + ((2.0 * l3) * x) / y, om)
    d2 = _div((3.0 * t + (5.0 * x) * d1) + ((2.0 * (1.0 - l2)) * l3) / y3, om)
    d3 = _div(((7.0 * x) * d2 + 8.0 * d1) - (((6.0 * (1.0 - l2)) * l5) * x) / y5, om)
    return d1, d2, d3


def _halley(p0, t0, ll, tol, max_iter, mg):
    for _ in range(max_iter):
        y = _y(p0, ll)
        d1, d2, d3 = _derivs(p0, y, t0, ll)
        if abs(d2) < 1e-14:
            raise _Stop(LambertStatus.TOO_CLOSE)
        p = p0 - _div((2.0 * d1) * d2, 2.0 * (d2 * d2) - d1 * d3)
        thr = tol * abs(p0) + tol
        mg.cmp(abs(p - p0), thr)
        if abs(p - p0) < thr:
            return p
        p0 = p
    raise _Stop(LambertStatus.MAX_ITER)


def _householder(p0, t0, ll, m, tol, max_iter, mg):
    """(x, steps taken, T'(x_last), the last step's T)"""
    for it in range(1, max_iter + 1):
        y = _y(p0, ll)
        t = time_of_flight(p0, y, ll, m, mg)
        fval = t - t0
        d1, d2, d3 = _derivs(p0, y, t, ll)
        num = d1 * d1 - (fval * d2) / 2.0
        den = d1 * (d1 * d1 - fval * d2) + (d3 * (fval * fval)) / 6.0
        if abs(den) < 1e-14:
            raise _Stop(LambertStatus.TOO_CLOSE)
        p = p0 - fval * (num / den)
        thr = tol * abs(p0) + tol
        mg.cmp(abs(p - p0), thr)
        if abs(p - p0) < thr:
            return p, it, d1
        p0 = p
    raise _Stop(LambertStatus.MAX_ITER)


def _t_min(ll, m, tol, max_iter, mg):
    if abs(ll - 1.0) < 1e-9:
        return time_of_flight(0.0, _y(0.0, ll), ll, m)
    x_i = 0.1
    t_i = time_of_flight(x_i, _y(x_i, ll), ll, m)
    x_min = _halley(x_i, t_i, ll, tol, max_iter, mg)
    return time_of_flight(x_min, _y(x_min, ll), ll, m)


def _initial_guess(t, ll, m, high_path, mg):
    if m == 0:
        l2 = ll * ll
        l3 = l2 * ll
        l5 = (l2 * l2) * ll
        t_0 = math.acos(ll) + ll * _sqrt(1.0 - l2)
        t_1 = (2.0 * (1.0 - l3)) / 3.0
        mg.cmp(t, t_0)
        mg.cmp(t, t_1)
        if t >= t_0:
            return math.pow(t_0 / t, _TWO_THIRDS) - 1.0
        if t < t_1:
            return ((((2.5 * t_1) / t) * (t_1 - t)) / (1.0 - l5)) + 1.0
        return math.exp((_LN2 * math.log(t / t_0)) / math.log(t_1 / t_0)) - 1.0
    mf = float(m)
    term_l = math.pow((mf * _PI + _PI) / (8.0 * t), _TWO_THIRDS)
    x_l = (term_l - 1.0) / (term_l + 1.0)
    term_r = math.pow((8.0 * t) / (mf * _PI), _TWO_THIRDS)
    x_r = (term_r - 1.0) / (term_r + 1.0)
    if high_path:
        return x_l if x_l < x_r else x_r
    return x_l if x_l > x_r else x_r


def _norm3(a):
    return math.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


N_VALUES = len(LambertParameter)


def solve(rv1, rv2, tof_s: float, mu: float, way=TransferKind.Auto, n_revs: int = 0, high_path: int = 0, tol: float = DEFAULT_TOL,
          max_iter: int = DEFAULT_MAX_ITER):
    """One problem, every parameter: (status, values[16], extras).  `rv1` / `rv2` are the bodies' states (6 components; the velocities
    only enter C3 .. DvTotal).  `extras` holds what the device test needs of the definition: `decision_margin`, `dT_dx` (T' at the last
    Householder step), `T`, `lam`, and `dv_dx` (the derivative of the six velocity components by x)."""
    rv1 = [float(v) for v in rv1]
    rv2 = [float(v) for v in rv2]
    tof_s, mu = float(tof_s), float(mu)
    m = int(n_revs)
    mg = _Margin()
    values = np.full(N_VALUES, _NAN)
    extras = {"decision_margin": math.inf}
    if not all(math.isfinite(v) for v in rv1 + rv2 + [tof_s]):
        return LambertStatus.BAD_INPUT, values, extras
    r1, r2 = rv1[:3], rv2[:3]
    n1, n2 = _norm3(r1), _norm3(r2)
    if n1 == 0.0 or n2 == 0.0 or not tof_s > 0.0:
        return LambertStatus.BAD_INPUT, values, extras
    c = _norm3((r2[0] - r1[0], r2[1] - r1[1], r2[2] - r1[2]))
    s = ((n1 + n2) + c) * 0.5
    i1 = (r1[0] / n1, r1[1] / n1, r1[2] / n1)
    i2 = (r2[0] / n2, r2[1] / n2, r2[2] / n2)
    h = _cross(i1, i2)
    hm = _norm3(h)
    if c == 0.0 or hm == 0.0:
        return LambertStatus.DEGENERATE, values, extras
    ih = (h[0] / hm, h[1] / hm, h[2] / hm)
    lam = _sqrt(1.0 - c / s)
    if int(way) == TransferKind.Auto:
        dnu = math.atan2(r2[1], r2[0]) - math.atan2(r1[1], r1[0])
        if dnu < 0.0:
            dnu = dnu + 2.0 * _PI
        mg.cmp(dnu, _PI)
        long_way = dnu > _PI
    else:
        long_way = int(way) == TransferKind.LongWay
    if long_way:
        ll = -lam
        t1, t2 = _cross(i1, ih), _cross(i2, ih)
    else:
        ll = lam
        t1, t2 = _cross(ih, i1), _cross(ih, i2)
    nt1, nt2 = _norm3(t1), _norm3(t2)
    t1 = (t1[0] / nt1, t1[1] / nt1, t1[2] / nt1)
    t2 = (t2[0] / nt2, t2[1] / nt2, t2[2] / nt2)
    big_t = math.sqrt((2.0 * mu) / ((s * s) * s)) * tof_s
    try:
        # find_xy
        m_max = math.floor(big_t / _PI)
        mg.cmp(big_t / _PI, m_max)
        mg.cmp(big_t / _PI, m_max + 1.0)
        t_00 = math.acos(ll) + ll * _sqrt(1.0 - ll * ll)
        if m_max > 0.0:
            edge = t_00 + m_max * _PI
            if m > 0:
                mg.cmp(big_t, edge)
            if big_t < edge:
                t_min = _t_min(ll, int(min(m_max, 2.0**31)), tol, max_iter, mg if m > 0 else _Margin())
                if m > 0:
                    mg.cmp(big_t, t_min)
                if big_t < t_min:
                    m_max = m_max - 1.0
        if float(m) > m_max:
            raise _Stop(LambertStatus.NOT_FEASIBLE)
        x0 = _initial_guess(big_t, ll, m, high_path, mg)
        x, iters, d1 = _householder(x0, big_t, ll, m, tol, max_iter, mg)
    except _Stop as stop:
        extras["decision_margin"] = mg.least
        return stop.status, values, extras
    y = _y(x, ll)
    gamma = math.sqrt((mu * s) / 2.0)
    rho = (n1 - n2) / c
    sigma = _sqrt(1.0 - rho * rho)
    a, b = ll * y - x, ll * y + x
    v_r1 = (gamma * (a - rho * b)) / n1
    v_r2 = ((-gamma) * (a + rho * b)) / n2
    v_t1 = ((gamma * sigma) * (y + ll * x)) / n1
    v_t2 = ((gamma * sigma) * (y + ll * x)) / n2
    v1 = [v_r1 * i1[k] + v_t1 * t1[k] for k in range(3)]
    v2 = [v_r2 * i2[k] + v_t2 * t2[k] for k in range(3)]
    cosd = (i1[0] * i2[0] + i1[1] * i2[1]) + i1[2] * i2[2]
    ang = math.acos(-1.0 if cosd < -1.0 else (1.0 if cosd > 1.0 else cosd)) * _TO_DEG
    if long_way:
        ang = 360.0 - ang
    ang = ang + 360.0 * float(m)
    w = (v1[0] - rv1[3], v1[1] - rv1[4], v1[2] - rv1[5])
    c3 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    vinf_dep = math.sqrt(c3)
    u = (rv2[3] - v2[0], rv2[4] - v2[1], rv2[5] - v2[2])
    vinf_arr = _norm3(u)
    ratio = w[2] / vinf_dep if vinf_dep != 0.0 else _NAN
    P = LambertParameter
    values[P.V1X:P.V1Z + 1] = v1
    values[P.V2X:P.V2Z + 1] = v2
    values[P.X], values[P.Iterations], values[P.TofS], values[P.TransferAngleDeg] = x, float(iters), tof_s, ang
    values[P.C3], values[P.VinfDep] = c3, vinf_dep
    values[P.DlaDeg] = math.asin(ratio) * _TO_DEG if -1.0 <= ratio <= 1.0 else _NAN
    values[P.RlaDeg] = math.atan2(w[1], w[0]) * _TO_DEG
    values[P.VinfArr], values[P.DvTotal] = vinf_arr, vinf_dep + vinf_arr
    # the derivative of the velocities by x (y' = lam^2 x / y), for the device test's bound
    dy = (ll * ll) * x / y
    da, db, dt_ = ll * dy - 1.0, ll * dy + 1.0, dy + ll
    dvr1, dvr2 = gamma * (da - rho * db) / n1, -gamma * (da + rho * db) / n2
    dvt1, dvt2 = gamma * sigma * dt_ / n1, gamma * sigma * dt_ / n2
    extras.update(decision_margin=mg.least, dT_dx=d1, T=big_t, lam=ll,
                  dv_dx=np.array([dvr1 * i1[k] + dvt1 * t1[k] for k in range(3)] + [dvr2 * i2[k] + dvt2 * t2[k] for k in range(3)]))
    return LambertStatus.OK, values, extras


@dataclass
class LambertSolution:
    """One solved problem, after the reference's `LambertSolution`: the same accessors with the same sign conventions."""

    v_init_km_s: np.ndarray
    v_final_km_s: np.ndarray
    rv1: np.ndarray
    rv2: np.ndarray
    values: np.ndarray
    status: LambertStatus
    decision_margin: float
    phi_rad: float = 0.0

    def of(self, param) -> float:
        return float(self.values[int(lambert_param(param))])

    @property
    def iterations(self) -> int:
        return int(self.of(LambertParameter.Iterations))

    def v_inf_outgoing_km_s(self) -> np.ndarray:
        return self.rv1[3:] - self.v_init_km_s

    def v_inf_incoming_km_s(self) -> np.ndarray:
        return self.rv2[3:] - self.v_final_km_s

    def v_inf_outgoing_declination_deg(self) -> float:
        return self.of(LambertParameter.DlaDeg)

    def v_inf_outgoing_right_ascension_deg(self) -> float:
        return self.of(LambertParameter.RlaDeg)

    def c3_km2_s2(self) -> float:
        return self.of(LambertParameter.C3)

    def transfer_orbit(self) -> np.ndarray:
        return np.concatenate([self.rv1[:3], self.v_init_km_s])

    def arrival_orbit(self) -> np.ndarray:
        return np.concatenate([self.rv2[:3], self.v_final_km_s])


def izzo(rv1, rv2, tof_s: float, mu_km3_s2: float, kind=TransferKind.Auto, n_revs: int = 0, high_path: int = 0, tol: float = DEFAULT_TOL,
         max_iter: int = DEFAULT_MAX_ITER) -> LambertSolution:
    """One Lambert problem on the host.  `rv1` / `rv2`: the departure and arrival bodies' states (3 or 6 components, km and km/s).
    A problem that cannot be solved raises ValueError naming its LambertStatus."""
    way, n_revs, high_path, tol, max_iter = check_solver(kind, n_revs, high_path, tol, max_iter)
    rv1 = np.concatenate([np.asarray(rv1, dtype=np.float64), np.zeros(3)])[:6]
    rv2 = np.concatenate([np.asarray(rv2, dtype=np.float64), np.zeros(3)])[:6]
    status, values, extras = solve(rv1, rv2, tof_s, mu_km3_s2, way, n_revs, high_path, tol, max_iter)
    if status != LambertStatus.OK:
        raise ValueError(f"lambert: {LambertStatus(status).name}")
    return LambertSolution(values[0:3].copy(), values[3:6].copy(), rv1, rv2, values, LambertStatus(status), extras["decision_margin"])


def batch_definition(rv1, rv2, tof_s, mu: float, way=TransferKind.Auto, n_revs: int = 0, high_path: int = 0, tol: float = DEFAULT_TOL,
                     max_iter: int = DEFAULT_MAX_ITER):
    """`solve` over component-major arrays rv1[6, n], rv2[6, n], tof_s[n]: (values[16, n], status[n], extras[n])."""
    rv1, rv2, tof_s = np.asarray(rv1, dtype=np.float64), np.asarray(rv2, dtype=np.float64), np.asarray(tof_s, dtype=np.float64)
    n = tof_s.shape[0]
    values, status, extras = np.full((N_VALUES, n), _NAN), np.zeros(n, dtype=np.int32), []
    for i in range(n):
        st, val, ex = solve(rv1[:, i], rv2[:, i], tof_s[i], mu, way, n_revs, high_path, tol, max_iter)
        status[i], values[:, i] = int(st), val
        extras.append(ex)
    return values, status, extras


def check_chain(what: str, naif_id: int, almanac, central):
    return chains.checked_chain(body_chain(naif_id, almanac, central), almanac, f"lambert_grid: the {what}")


def chain_state(chain, et_s, almanac):
    """The signed sum of a chain at the epochs `et_s` (seconds), in chain order, from zero: (rv[..., 6], inside[...])."""
    r, v, inside = chains.chain_state(chain, et_s, almanac)
    return np.concatenate([r, v], axis=-1), inside


def grid_epochs(n_dep, n_arr, dep0_ns, dep_step_ns, arr0_ns=None, arr_step_ns=None, tof0_ns=None, tof_step_ns=None):
    """(dep_ns[n_dep], arr_ns[n_dep, n_arr]) of a grid: arrivals by epoch (`arr0_ns`), or by time of flight (`tof0_ns`)."""
    dep = np.int64(dep0_ns) + np.arange(n_dep, dtype=np.int64) * np.int64(dep_step_ns)
    if tof0_ns is not None:
        arr = dep[:, None] + (np.int64(tof0_ns) + np.arange(n_arr, dtype=np.int64) * np.int64(tof_step_ns))[None, :]
    else:
        arr = np.broadcast_to((np.int64(arr0_ns) + np.arange(n_arr, dtype=np.int64) * np.int64(arr_step_ns))[None, :], (n_dep, n_arr))
    return dep, np.ascontiguousarray(arr)


def grid_states(dep_body, arr_body, centre, dep_ns, arr_ns, almanac, central):
    """The bodies' states about `centre` at the grid's epochs: chain(body) - chain(centre), component by component:
    (rv1[n_dep, 6], rv2[n_dep, n_arr, 6], inside[n_dep, n_arr])."""
    cd, ca, cc = (check_chain(w, b.naif_id, almanac, central) for w, b in (("departure body", dep_body), ("arrival body", arr_body), ("centre", centre)))
    if cd == cc or ca == cc:
        raise ValueError("lambert_grid: a body whose chain is the centre's has radius zero by construction")
    et_d, et_a = _ns_to_seconds(dep_ns), _ns_to_seconds(arr_ns)
    b1, in1 = chain_state(cd, et_d, almanac)
    c1, in1c = chain_state(cc, et_d, almanac)
    b2, in2 = chain_state(ca, et_a, almanac)
    c2, in2c = chain_state(cc, et_a, almanac)
    return b1 - c1, b2 - c2, (in1 & in1c)[:, None] & in2 & in2c


def grid_definition(dep_body, arr_body, centre, almanac, central, n_dep, n_arr, dep0_ns, dep_step_ns, arr0_ns=None, arr_step_ns=None,
                    tof0_ns=None, tof_step_ns=None, way=TransferKind.Auto, n_revs: int = 0, high_path: int = 0, tol: float = DEFAULT_TOL,
                    max_iter: int = DEFAULT_MAX_ITER):
    """The porkchop on the host: (values[16, n_dep, n_arr], status[n_dep, n_arr], extras[n_dep][n_arr], dep_ns, arr_ns).  `centre.mu_km3_s2`
    is the gravitational parameter; a cell with an epoch outside a chain's segments is EPHEM_RANGE, one whose arrival is not after
    its departure BAD_INPUT."""
    dep_ns, arr_ns = grid_epochs(n_dep, n_arr, dep0_ns, dep_step_ns, arr0_ns, arr_step_ns, tof0_ns, tof_step_ns)
    rv1, rv2, inside = grid_states(dep_body, arr_body, centre, dep_ns, arr_ns, almanac, central)
    tof = _ns_to_seconds(arr_ns - dep_ns[:, None])
    values, status = np.full((N_VALUES, n_dep, n_arr), _NAN), np.zeros((n_dep, n_arr), dtype=np.int32)
    extras = [[None] * n_arr for _ in range(n_dep)]
    for i in range(n_dep):
        for j in range(n_arr):
            if not inside[i, j]:
                status[i, j], extras[i][j] = int(LambertStatus.EPHEM_RANGE), {"decision_margin": math.inf}
                continue
            st, val, ex = solve(rv1[i], rv2[i, j], tof[i, j], float(centre.mu_km3_s2), way, n_revs, high_path, tol, max_iter)
            status[i, j], values[:, i, j], extras[i][j] = int(st), val, ex
    return values, status, extras, dep_ns, arr_ns


class LambertGrid:
    """What `GpuContext.lambert_grid` (and `lambert_batch`, as a grid of one row) returns: values[P, n_dep, n_arr] by parameter, the
    status of every cell, and the epochs."""

    def __init__(self, params, values: np.ndarray, status: np.ndarray, dep_ns=None, arr_ns=None):
        self.params = [lambert_param(p) for p in params]
        self.values, self.status, self.dep_ns, self.arr_ns = values, status, dep_ns, arr_ns

    def of(self, param) -> np.ndarray:
        return self.values[self.params.index(lambert_param(param))]

    @property
    def feasible_fraction(self) -> float:
        return float((self.status == 0).mean()) if self.status.size else 0.0

    def best(self, param):
        """The cell of least `param` among the solved ones: (value, index tuple, departure epoch, arrival epoch); None when no cell is solved."""
        vals = np.where(self.status == 0, self.of(param), np.inf)
        if not self.status.size or not np.isfinite(vals).any():
            return None
        idx = np.unravel_index(int(np.argmin(vals)), vals.shape)
        dep = None if self.dep_ns is None else int(self.dep_ns[idx[0]])
        arr = None if self.arr_ns is None else int(self.arr_ns[idx])
        return float(vals[idx]), tuple(int(k) for k in idx), dep, arr
