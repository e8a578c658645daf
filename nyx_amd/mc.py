"""Monte Carlo front end of the batched propagation path.

Mirror of the reference's `MonteCarlo` (nyx-core/src/mc/montecarlo.rs:44-296) at the level this path
needs it: states are generated on the host, one by one, from a single seeded stream
(`generate_states`, montecarlo.rs:277-296; the index is the position AFTER the skip, as there), run `index` keeps its dispersed state
(`Run{index, dispersed_state, result}`, mc/results.rs:48-59), `resume_run_until_epoch(skip, ..)`
regenerates the stream and skips the first `skip` samples (montecarlo.rs:208-224).  Where the reference
hands the states to a rayon `par_iter` (montecarlo.rs:233-253), this hands the whole batch to the GPU
through the C-ABI; with several ranks the ensemble is split into contiguous index shards and the
final states are collected with one all-gather (RCCL on GPUs, gloo in the CPU tests).

The random stream is the reference's (`rand_pcg::Pcg64Mcg::new(seed)` + ziggurat `Normal(0, 1)`, nine draws per
state: nyx_amd/rng.py, pinned by the reference's seeded known-answer tests).  What is NOT pinned is the orientation of
the covariance factor: the reference takes `V sqrt(S)` from nalgebra's `svd_unordered`, whose column order and signs for
repeated or zero singular values are nalgebra's own; here a diagonal covariance maps component k to draw k (which is what
the reference's seeded tests show for diagonal cases) and a general one goes through LAPACK's SVD - the same
distribution, possibly another labelling of the draws.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, List, Optional, Sequence

import copy
import os

import numpy as np

from . import _abi
from .rng import Pcg64Mcg
from .params import FRAME_OF, StateError, StateParameter, ric_difference, smooth_ric, state_value
from .groundtrack import DEFAULT_PARAMS as GROUND_TRACK_DEFAULT, GroundTrackParameter, body_fixed_value, check_frame, to_body_fixed
from .stations import DEFAULT_PARAMS as AER_DEFAULT, AerParameter, check_stations, sez_value, station_consts
from .eclipse import DEFAULT_PARAMS as ECLIPSE_DEFAULT, EclipseParameter, check_shadow_model, eclipse_value, state_changes
from .frames import FrameParameter, check_target, frame_param, frame_value
from .links import DEFAULT_PARAMS as LINK_DEFAULT, LinkParameter, check_link_bodies, default_bodies, link_param, link_value, outside_ephemerides
from .propagator import Almanac, Propagator, Spacecraft, Traj, ric_bounds, series_bounds
from . import stats as series_statistics

# indices into the 9-vector [x, y, z, vx, vy, vz, Cr, Cd, prop mass] (cosmic/spacecraft.rs:451-473)
STATE_DIM = 9


@dataclass
class StateDispersion:
    """mc/dispersion.rs:29-48."""

    param: StateParameter
    mean: Optional[float] = None
    std_dev: Optional[float] = None

    @classmethod
    def zero_mean(cls, param: StateParameter, std_dev: float):
        return cls(param, 0.0, std_dev)


_ORBITAL = {StateParameter.X, StateParameter.Y, StateParameter.Z, StateParameter.VX, StateParameter.VY, StateParameter.VZ,
            StateParameter.Rmag, StateParameter.Vmag, StateParameter.Hmag, StateParameter.Energy, StateParameter.SemiMajorAxis,
            StateParameter.Eccentricity, StateParameter.Inclination, StateParameter.RAAN, StateParameter.AoP,
            StateParameter.TrueAnomaly, StateParameter.Period, StateParameter.ApoapsisRadius, StateParameter.PeriapsisRadius}


def _partials(param: StateParameter, rv: np.ndarray, mu: float) -> np.ndarray:
    """d param / d (x, y, z, vx, vy, vz) at `rv`.  The reference reads them off ANISE's `OrbitGrad` (hyperdual numbers,
    absent here): exact for the Cartesian components and the magnitudes, central differences for the Keplerian elements."""
    cart = [StateParameter.X, StateParameter.Y, StateParameter.Z, StateParameter.VX, StateParameter.VY, StateParameter.VZ]
    g = np.zeros(6)
    if param in cart:
        g[cart.index(param)] = 1.0
    elif param is StateParameter.Rmag:
        g[:3] = rv[:3] / np.linalg.norm(rv[:3])
    elif param is StateParameter.Vmag:
        g[3:] = rv[3:] / np.linalg.norm(rv[3:])
    else:
        for k in range(6):
            h = 1e-6 * (np.linalg.norm(rv[:3]) if k < 3 else np.linalg.norm(rv[3:]))
            up, dn = rv.copy(), rv.copy()
            up[k] += h
            dn[k] -= h
            d = state_value(param, up, mu) - state_value(param, dn, mu)
            if param in (StateParameter.RAAN, StateParameter.AoP, StateParameter.TrueAnomaly):
                d = (d + 180.0) % 360.0 - 180.0
            g[k] = d / (2.0 * h)
    return g


class MvnSpacecraft:
    """Multivariate normal over the 9-state: x = L z + mean, z ~ N(0, I) (mc/multivariate.rs:63-330); L = V sqrt(S) from the
    SVD of the 9x9 covariance (`sqrt_s_v`, multivariate.rs:203-218, 262-272).  Built from a covariance (`from_spacecraft_cov`,
    the constructor; `from_sigmas` for a diagonal one) or from dispersions of state parameters (`new` / `zero_mean`)."""

    def __init__(self, template: Spacecraft, cov: np.ndarray, mean: Optional[np.ndarray] = None, dispersions=None):
        self.template = template
        c = np.zeros((STATE_DIM, STATE_DIM))
        cov = np.asarray(cov, dtype=np.float64)
        c[: cov.shape[0], : cov.shape[1]] = cov
        if np.any(np.linalg.eigvalsh(0.5 * (c + c.T)) < -1e-12 * max(1.0, float(np.abs(c).max()))):
            raise ValueError("covariance matrix is not positive semi-definite")   # NyxError::CovarianceMatrixNotPsd
        self.cov = c
        if np.count_nonzero(c - np.diag(np.diagonal(c))) == 0:
            self._sqrt_s_v = np.diag(np.sqrt(np.diagonal(c)))   # V = I: component k takes draw k
        else:
            _, sv, vt = np.linalg.svd(c)
            self._sqrt_s_v = vt.T * np.sqrt(sv)[None, :]
        m = np.zeros(STATE_DIM)
        if mean is not None:
            m[: len(mean)] = mean
        self._mean = m
        self.mean = m
        if dispersions is None:   # from_spacecraft_cov lists the nine components (multivariate.rs:274-312: std_dev <- the VARIANCE)
            dispersions = [StateDispersion(p, None, float(c[k, k])) for k, p in enumerate(_VECTOR_PARAMS)]
        self.dispersions = list(dispersions)

    from_spacecraft_cov = classmethod(lambda cls, template, cov, mean=None: cls(template, cov, mean))

    @classmethod
    def from_sigmas(cls, template: Spacecraft, sigmas: Sequence[float]):
        s = np.zeros(STATE_DIM)
        s[: len(sigmas)] = sigmas
        return cls(template, np.diag(s ** 2))

    @classmethod
    def new(cls, template: Spacecraft, dispersions: Sequence[StateDispersion]):
        """multivariate.rs:78-226: the dispersions of orbital parameters are independent in THEIR space; the Jacobian J of the
        parameters w.r.t. the Cartesian state maps them back, C = J+ P J+^T with J+ the pseudo-inverse, mean = J+ means."""
        dispersions = list(dispersions)
        cov = np.zeros((STATE_DIM, STATE_DIM))
        mean = np.zeros(STATE_DIM)
        orbital = [d for d in dispersions if d.param in _ORBITAL]
        if orbital:
            rv = np.asarray(template.rv, dtype=np.float64)
            jac = np.stack([_partials(d.param, rv, float(template.frame.mu_km3_s2)) for d in orbital])
            p = np.diag([(d.std_dev or 0.0) ** 2 for d in orbital])
            means = np.array([d.mean or 0.0 for d in orbital])
            jac_inv = np.linalg.pinv(jac)
            cov[:6, :6] = jac_inv @ p @ jac_inv.T
            mean[:6] = jac_inv @ means
        for d in dispersions:
            if d.param in _ORBITAL:
                continue
            # as written in the reference (multivariate.rs:183-197): the variance is taken from `mean`, Cr lands in slot 7 and
            # Cd in slot 8 of [.., Cr, Cd, prop mass]; the mass branch indexes (9, 9) of a 9x9 matrix and panics
            if d.param is StateParameter.Cr:
                cov[7, 7] = (d.mean or 0.0) ** 2
            elif d.param is StateParameter.Cd:
                cov[8, 8] = (d.mean or 0.0) ** 2
            elif d.param in (StateParameter.DryMass, StateParameter.PropMass):
                raise IndexError("Matrix index out of bounds (multivariate.rs:193: cov[(9, 9)] of a 9x9)")
            else:
                raise StateError(d.param)   # StateError::ReadOnly
        return cls(template, cov, mean, dispersions)

    @classmethod
    def zero_mean(cls, template: Spacecraft, dispersions: Sequence[StateDispersion]):
        return cls.new(template, [StateDispersion(d.param, 0.0, d.std_dev) for d in dispersions])

    def sample_vector(self, rng) -> np.ndarray:
        """multivariate.rs:300-303: nine standard normals, in order, from the run's stream (`rng`: nyx_amd.rng.Pcg64Mcg, or a
        numpy Generator)."""
        z = np.array(rng.normal_vector(STATE_DIM)) if hasattr(rng, "normal_vector") else rng.standard_normal(STATE_DIM)
        return self._sqrt_s_v @ z + self._mean

    def disperses(self, k: int) -> bool:
        """Is component k of the 9-vector dispersed (non-zero variance or mean)?"""
        return bool(np.any(self._sqrt_s_v[k] != 0.0) or self._mean[k] != 0.0)


# the dispersed components of the 9-vector, as state parameters (multivariate.rs:298-330)
_VECTOR_PARAMS = [StateParameter.X, StateParameter.Y, StateParameter.Z, StateParameter.VX, StateParameter.VY, StateParameter.VZ,
                  StateParameter.Cr, StateParameter.Cd, StateParameter.PropMass]


class DispersedState(Spacecraft):
    """generator.rs:59-67: the dispersed state plus `actual_dispersions`, the list of (parameter, delta).  The delta is
    `template.value(param) - state.value(param)` - template MINUS dispersed, as the reference computes it
    (multivariate.rs:320-325).  Subclass of Spacecraft so that it packs like one (`.state` returns itself)."""

    actual_dispersions: list = []

    @property
    def state(self) -> "Spacecraft":
        return self


class PropResult:
    """results.rs:73-80: the final state of a run and its trajectory.  `traj` is None when the run was made without
    dense output (`with_traj=False`) or on another rank of a sharded ensemble.  Attribute access falls through to the
    state, so `run.result.rv` and `run.result.state.rv` are the same thing."""

    def __init__(self, state: Spacecraft, traj_src=None):
        self.state = state
        self._traj_src = traj_src   # (context, TrajBatch, row) - the Traj object is built on first use
        self._traj = None

    @property
    def traj(self) -> Optional[Traj]:
        if self._traj is None and self._traj_src is not None:
            ctx, batch, row = self._traj_src
            self._traj = Traj(ctx, batch, row)
        return self._traj

    def __getattr__(self, name):
        if name.startswith("_") or name in ("state", "traj"):
            raise AttributeError(name)
        return getattr(self.state, name)


@dataclass
class Run:
    index: int
    dispersed_state: DispersedState
    result: object  # PropResult or PropagationError


class _Series:
    """What the series of the array reports share (`of`: those with `params`).  No field of its own: the dataclasses below keep
    theirs, and their order."""

    def epochs(self, j: int) -> np.ndarray:
        return int(self.epoch0_ns[j]) + int(self.step_ns) * np.arange(int(self.len[j]), dtype=np.int64)

    def of(self, param) -> np.ndarray:
        """values[K, runs] of one parameter."""
        return self.values[self.params.index(param)]


@dataclass
class ValueSeries(_Series):
    """`Results.values_of`: sample k of run j (position in `Results.runs`) of parameter p is `values[p, k, j]`, taken at
    `epoch0_ns[j] + k * step_ns`; `len[j]` samples are valid, the slots after them NaN.  A failed run (`ok[j]` False) has
    len 0 and holds the caller's substitute in every slot."""

    params: list
    values: np.ndarray      # [P, K, runs]
    len: np.ndarray         # [runs] int32
    epoch0_ns: np.ndarray   # [runs] int64
    step_ns: int
    ok: np.ndarray          # [runs] bool

    def flat(self, param, value_if_run_failed: Optional[float] = None) -> List[float]:
        """One parameter as the list reports lay it out (results.rs:86-160): run after run; a failed run is skipped, or
        stands for ONE `value_if_run_failed`."""
        p = self.params.index(param)
        out: List[float] = []
        for j in range(self.values.shape[2]):
            if self.ok[j]:
                out.extend(self.values[p, :int(self.len[j]), j].tolist())
            elif value_if_run_failed is not None:
                out.append(float(value_if_run_failed))
        return out


@dataclass
class RicSeries(_Series):
    """`Results.ric_dispersions`: component c (dR, dI, dC in km, dvR, dvI, dvC in km/s) of sample k of run j (position in
    `Results.runs`) is `values[c, k, j]`, taken at `epoch0_ns[j] + k * step_ns`; `len[j]` samples are valid, the slots after
    them NaN.  A failed run (`ok[j]` False) is a column of NaN with len 0.  `count[k]` runs have sample k; `mean[k]` and the
    unbiased `cov[k]` are taken over them (NaN where count < 1 / < 2).  They are indexed by SAMPLE: a time series of the
    ensemble when all `epoch0_ns` agree - every run and the nominal starting at one epoch, the Monte Carlo case.
    (No `params` here, so `of` does not apply: component c is `values[c]`.)"""

    values: np.ndarray      # [6, K, runs]
    len: np.ndarray         # [runs] int32
    epoch0_ns: np.ndarray   # [runs] int64
    step_ns: int
    ok: np.ndarray          # [runs] bool
    count: np.ndarray       # [K]
    mean: np.ndarray        # [K, 6]
    cov: np.ndarray         # [K, 6, 6]
    moments: np.ndarray     # [K, 28] what they are made of: count, sum d[6], the row-major upper triangle of sum d d^T


@dataclass
class GroundTrackSeries(_Series):
    """`Results.ground_tracks`: sample k of run j (position in `Results.runs`) of parameter p is `values[p, k, j]`, taken at
    `epoch0_ns[j] + k * step_ns` in the body-fixed `frame`; `len[j]` samples are valid, the slots after them NaN.  A failed
    run (`ok[j]` False) is a column of NaN with len 0: an empty series."""

    params: list
    values: np.ndarray      # [P, K, runs]
    len: np.ndarray         # [runs] int32
    epoch0_ns: np.ndarray   # [runs] int64
    step_ns: int
    ok: np.ndarray          # [runs] bool
    frame: object = None


@dataclass
class AerSeries(_Series):
    """`Results.station_views`: sample k of run j (position in `Results.runs`) of parameter p seen from station s is
    `values[s, p, k, j]`, taken at `epoch0_ns[j] + k * step_ns`; `len[j]` samples are valid (the same for every station), the
    slots after them NaN.  A failed run (`ok[j]` False) is a column of NaN with len 0: an empty series."""

    stations: list
    params: list
    values: np.ndarray      # [S, P, K, runs]
    len: np.ndarray         # [runs] int32
    epoch0_ns: np.ndarray   # [runs] int64
    step_ns: int
    ok: np.ndarray          # [runs] bool

    def of(self, station, param) -> np.ndarray:
        """values[K, runs] of one parameter seen from one station (a GroundStation of `stations`, or its position)."""
        return self.values[self._station(station), self.params.index(param)]

    def _station(self, station) -> int:
        return int(station) if isinstance(station, (int, np.integer)) else [st is station for st in self.stations].index(True)

    def visible_fraction(self, station) -> np.ndarray:
        """[K]: per sample, the share of the runs HOLDING that sample (k < len[j]) whose elevation is at or above the mask of
        `station` (a GroundStation of `stations`, or its position); NaN where no run holds the sample.  Formed on the host from
        `Visible`, or from `ElevationAboveMask` / `Elevation` when that is what the series holds."""
        s = self._station(station)
        if AerParameter.Visible in self.params:
            seen = self.values[s, self.params.index(AerParameter.Visible)] > 0.0
        elif AerParameter.ElevationAboveMask in self.params:
            seen = self.values[s, self.params.index(AerParameter.ElevationAboveMask)] >= 0.0
        elif AerParameter.Elevation in self.params:
            seen = self.values[s, self.params.index(AerParameter.Elevation)] - float(self.stations[s].elevation_mask_deg) >= 0.0
        else:
            raise ValueError("visible_fraction: the series holds none of Visible, ElevationAboveMask and Elevation")
        held = np.arange(self.values.shape[2])[:, None] < self.len[None, :].astype(np.int64)
        count = held.sum(axis=1)
        with np.errstate(invalid="ignore", divide="ignore"):
            return (seen & held).sum(axis=1) / np.where(count > 0, count, np.nan)


@dataclass
class EclipseSeries(_Series):
    """`Results.eclipses`: sample k of run j (position in `Results.runs`) of parameter p is `values[p, k, j]`, taken at
    `epoch0_ns[j] + k * step_ns`; `len[j]` samples are valid, the slots after them NaN.  A failed run (`ok[j]` False) is a
    column of NaN with len 0: an empty series.  A parameter is an EclipseParameter or a pair (per-body parameter, body)."""

    model: object
    params: list
    values: np.ndarray      # [P, K, runs]
    len: np.ndarray         # [runs] int32
    epoch0_ns: np.ndarray   # [runs] int64
    step_ns: int
    ok: np.ndarray          # [runs] bool

    def _held(self) -> np.ndarray:
        return np.arange(self.values.shape[1])[:, None] < self.len[None, :].astype(np.int64)

    def _state(self) -> np.ndarray:
        """0 / 1 / 2 per slot, from `State`, or from `Occultation` when that is what the series holds."""
        if EclipseParameter.State in self.params:
            return self.of(EclipseParameter.State)
        if EclipseParameter.Occultation in self.params:
            occ = self.of(EclipseParameter.Occultation)
            return np.where(occ == 0.0, 0.0, np.where(occ == 100.0, 2.0, 1.0))
        raise ValueError("the series holds neither State nor Occultation")

    def _share(self, hit: np.ndarray) -> np.ndarray:
        held = self._held()
        count = held.sum(axis=0)
        with np.errstate(invalid="ignore", divide="ignore"):
            return (hit & held).sum(axis=0) / np.where(count > 0, count, np.nan)

    @property
    def shadow_fraction(self) -> np.ndarray:
        """[runs]: the share of the produced samples of a run that are not fully lit (State != 0); NaN for an empty series."""
        return self._share(self._state() != 0.0)

    @property
    def umbra_fraction(self) -> np.ndarray:
        """[runs]: the share of the produced samples of a run in the umbra (State == 2); NaN for an empty series."""
        return self._share(self._state() == 2.0)

    @property
    def state_changes(self) -> np.ndarray:
        """[runs]: the number of samples whose Occultation differs from the previous sample's (`eclipse.state_changes`)."""
        if EclipseParameter.Occultation not in self.params:
            raise ValueError("state_changes: the series does not hold Occultation")
        return state_changes(self.of(EclipseParameter.Occultation), self.len)


@dataclass
class FrameSeries(_Series):
    """`Results.frame_values`: sample k of run j (position in `Results.runs`) of parameter p, about `target`, is `values[p, k, j]`,
    taken at `epoch0_ns[j] + k * step_ns`; `len[j]` samples are valid, the slots after them NaN.  A failed run (`ok[j]` False) is a
    column of NaN with len 0: an empty series.  A held sample that is not hyperbolic about the target has NaN B-plane values."""

    target: object
    params: list            # FrameParameter members
    values: np.ndarray      # [P, K, runs]
    len: np.ndarray         # [runs] int32
    epoch0_ns: np.ndarray   # [runs] int64
    step_ns: int
    ok: np.ndarray          # [runs] bool

    def _held(self) -> np.ndarray:
        return np.arange(self.values.shape[1])[:, None] < self.len[None, :].astype(np.int64)

    def of(self, param) -> np.ndarray:
        """values[K, runs] of one parameter (a FrameParameter, or the StateParameter of the same name)."""
        return self.values[self.params.index(frame_param(param))]

    def closest_approach(self):
        """(sample[runs] int64, rmag[runs]): per run the sample index and the value of the minimum of `Rmag` over the run's `len`
        samples (the first one when several tie); (-1, NaN) for an empty series.  Raises when the series does not hold Rmag."""
        if FrameParameter.Rmag not in self.params:
            raise ValueError("closest_approach: the series does not hold Rmag")
        rmag = np.where(self._held(), self.of(FrameParameter.Rmag), np.inf)
        if rmag.shape[0] == 0:
            return np.full(rmag.shape[1], -1, dtype=np.int64), np.full(rmag.shape[1], np.nan)
        k = np.argmin(rmag, axis=0).astype(np.int64)
        best = rmag[k, np.arange(rmag.shape[1])]
        empty = self.len <= 0
        return np.where(empty, -1, k), np.where(empty, np.nan, best)

    def hyperbolic_fraction(self) -> np.ndarray:
        """[runs]: the share of the produced samples of a run that are hyperbolic about the target (a B-plane value, VInfinity or
        Eccentricity > 1 tells); NaN for an empty series.  Raises when the series holds none of them."""
        for p in (FrameParameter.BdotT, FrameParameter.BdotR, FrameParameter.BAngle, FrameParameter.BMagnitude, FrameParameter.VInfinity):
            if p in self.params:
                hyp = ~np.isnan(self.of(p))
                break
        else:
            if FrameParameter.Eccentricity not in self.params:
                raise ValueError("hyperbolic_fraction: the series holds neither a B-plane parameter, VInfinity nor Eccentricity")
            with np.errstate(invalid="ignore"):
                hyp = self.of(FrameParameter.Eccentricity) > 1.0
        held = self._held()
        count = held.sum(axis=0)
        with np.errstate(invalid="ignore", divide="ignore"):
            return (hyp & held).sum(axis=0) / np.where(count > 0, count, np.nan)


@dataclass
class LinkSeries(_Series):
    """`Results.link_views`: sample k of run j (position in `Results.runs`) of parameter p of the link from the transmitter to that
    run is `values[p, k, j]`, taken at `epoch0_ns[j] + k * step_ns`; `len[j]` samples are valid, the slots after them NaN.  A failed
    run (`ok[j]` False) is a column of NaN with len 0: an empty series.  A parameter is a LinkParameter or a pair (per-body
    parameter, body)."""

    bodies: list
    params: list
    values: np.ndarray      # [P, K, runs]
    len: np.ndarray         # [runs] int32
    epoch0_ns: np.ndarray   # [runs] int64
    step_ns: int
    ok: np.ndarray          # [runs] bool

    def _held(self) -> np.ndarray:
        return np.arange(self.values.shape[1])[:, None] < self.len[None, :].astype(np.int64)

    def visible_fraction(self) -> np.ndarray:
        """[K]: per sample, the share of the runs HOLDING that sample (k < len[j]) that see the transmitter, as
        `AerSeries.visible_fraction`; NaN where no run holds the sample.  Formed on the host from `Visible`, or from
        `ObstructingBody` / `Clearance` when that is what the series holds."""
        if LinkParameter.Visible in self.params:
            seen = self.of(LinkParameter.Visible) > 0.0
        elif LinkParameter.ObstructingBody in self.params:
            seen = self.of(LinkParameter.ObstructingBody) < 0.0
        elif LinkParameter.Clearance in self.params:
            seen = self.of(LinkParameter.Clearance) > 0.0
        else:
            raise ValueError("visible_fraction: the series holds none of Visible, ObstructingBody and Clearance")
        held = self._held()
        count = held.sum(axis=1)
        with np.errstate(invalid="ignore", divide="ignore"):
            return (seen & held).sum(axis=1) / np.where(count > 0, count, np.nan)

    def closest_range(self):
        """(range_km[runs], epoch_ns[runs] int64): per run the minimum of `Range` over the run's `len` samples and the epoch it is
        taken at (the first one when several tie); (NaN, 0) for an empty series.  Raises when the series does not hold Range."""
        if LinkParameter.Range not in self.params:
            raise ValueError("closest_range: the series does not hold Range")
        rng = np.where(self._held(), self.of(LinkParameter.Range), np.inf)
        runs = rng.shape[1]
        if rng.shape[0] == 0:
            return np.full(runs, np.nan), np.zeros(runs, dtype=np.int64)
        k = np.argmin(rng, axis=0).astype(np.int64)
        empty = self.len <= 0
        return np.where(empty, np.nan, rng[k, np.arange(runs)]), np.where(empty, 0, self.epoch0_ns + k * int(self.step_ns))


def _fill_head(head: np.ndarray, k: int, n_k: int, first_epoch_ns) -> None:
    """Row k of the head of an array report - what every rank must know of a successful run before the columns are gathered:
    its len, the bit pattern of its first epoch (0 for an empty series), and that it succeeded."""
    head[k, 0], head[k, 2] = n_k, 1.0
    head[k, 1:2] = np.array([first_epoch_ns if n_k else 0], dtype=np.int64).view(np.float64)


RIC_TRIU = np.triu_indices(6)
RIC_ROWS = ("dR", "dI", "dC", "dvR", "dvI", "dvC")

# the array reports `Results.series_stats` serves, and the evaluator's entry behind each
SERIES_REPORTS = {"values_of": "traj_values", "ric_dispersions": "traj_ric_diff", "ground_tracks": "traj_ground_track", "station_views": "traj_aer",
                  "eclipses": "traj_eclipse", "frame_values": "traj_frame_values", "link_views": "traj_link"}


class _StatsTap:
    """The evaluator of a Results for the length of one `series_stats`: everything is the evaluator's own but `entry`, which is
    called with `stats=` - the statistics (`stats`, `length`, `epoch0`) stay here, and the report that called gets an empty series
    of the right shape, so that nothing else of it has to know."""

    def __init__(self, ctx, entry: str, request):
        self._ctx, self._entry, self._request = ctx, entry, request
        self.stats = self.length = self.epoch0 = None

    def __getattr__(self, name):
        return getattr(self._ctx, name)

    def _tapped(self, tb, *args, **kwargs):
        kwargs.pop("moments", None)                          # (RIC's own sums are not asked for through the statistics)
        got = getattr(self._ctx, self._entry)(tb, *args, stats=self._request, **kwargs)
        self.stats, self.length = got[0], got[1]
        with_ref = self._entry in ("traj_link", "traj_ric_diff")
        self.epoch0 = got[2] if with_ref else series_bounds(tb, args[-2], args[-1])[0]
        none = np.empty(self.stats.shape[:-2] + (0, tb.n)), np.zeros(tb.n, dtype=np.int32)
        if self._entry == "traj_ric_diff":
            return none + (self.epoch0, np.zeros((0, _abi.RIC_MOMENTS)))
        return none + ((self.epoch0,) if with_ref else ())


for _entry in SERIES_REPORTS.values():
    setattr(_StatsTap, _entry, _StatsTap._tapped)


def ric_moments(cols, k_max: int) -> np.ndarray:
    """[k_max, 28]: per sample the count, sum d[6] and the row-major upper triangle of sum d d^T over the columns
    (d[6, len] each, None skipped) that have that sample - the layout of nyx_hip_traj_ric_diff's `moments`."""
    mom = np.zeros((k_max, _abi.RIC_MOMENTS))
    for col in cols:
        if col is None:
            continue
        d = col.T[:k_max]
        m = len(d)
        mom[:m, 0] += 1.0
        mom[:m, 1:7] += d
        mom[:m, 7:] += (d[:, :, None] * d[:, None, :])[:, RIC_TRIU[0], RIC_TRIU[1]]
    return mom


def ric_mean_cov(mom: np.ndarray):
    """(count[K], mean[K, 6], cov[K, 6, 6]) of moments[K, 28]: mean = s / n, cov = (S - n m m^T) / (n - 1)."""
    k_n = len(mom)
    count = mom[:, 0].copy()
    sxx = np.zeros((k_n, 6, 6))
    sxx[:, RIC_TRIU[0], RIC_TRIU[1]] = mom[:, 7:]
    sxx[:, RIC_TRIU[1], RIC_TRIU[0]] = mom[:, 7:]
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(count[:, None] >= 1, mom[:, 1:7] / count[:, None], np.nan)
        cov = (sxx - count[:, None, None] * mean[:, :, None] * mean[:, None, :]) / (count[:, None, None] - 1.0)
    cov[count < 2] = np.nan
    return count, mean, cov


@dataclass
class Results:
    """mc/results.rs:60-245.  Runs are sorted by index.  When the runs of this process carry trajectories they share one
    dense-output batch, and the `every_value_of*` reports resample ALL of them with one launch of the trajectory kernel
    (`Traj::every` per run in the reference, results.rs:134-160)."""

    runs: List[Run]
    scenario: str
    mu_km3_s2: float = 0.0
    _traj_ctx: object = field(default=None, repr=False)
    _traj_batch: object = field(default=None, repr=False)
    _traj_rows: dict = field(default_factory=dict, repr=False)   # run index -> row of the dense-output batch
    # sharded ensemble: the process group and the positions [lo, hi) of `runs` this rank propagated (and holds trajectories of)
    _dist: object = field(default=None, repr=False)
    _local: Optional[tuple] = field(default=None, repr=False)

    def ok_runs(self) -> List[Run]:
        return [r for r in self.runs if isinstance(r.result, PropResult)]

    def final_rv(self) -> np.ndarray:
        return np.array([r.result.state.rv for r in self.ok_runs()])

    def _local_runs(self) -> List[Run]:
        return self.runs if self._local is None else self.runs[self._local[0]:self._local[1]]

    def mean_and_covariance(self):
        """Ensemble mean and (unbiased) covariance of the final 9-vectors [r, v, Cr, Cd, prop mass] of the successful runs
        (NINE components since round 2: Cr, Cd and the propellant mass are dispersed and integrated like r and v; rounds before
        returned the 6-vector only).  No successful run at all: NaNs.
        On a sharded ensemble each rank sums ITS runs only and one all-reduce (RCCL / gloo) of the 1 + 9 + 45 moments
        [count, sum(x - x0), upper triangle of sum((x - x0)(x - x0)^T)] completes them; x0 = the final state of the
        first successful run (every rank holds the gathered final states), which keeps the sums well conditioned.
        Returns (mean[9], cov[9, 9])."""
        d = STATE_DIM
        iu = np.triu_indices(d)
        err, mom, x0 = None, np.zeros(1 + d + len(iu[0])), np.zeros(d)
        try:
            ok = self.ok_runs()
            x0 = _vec9(ok[0].result.state) if ok else np.zeros(d)
            xs = np.array([_vec9(r.result.state) for r in self._local_runs() if isinstance(r.result, PropResult)]).reshape(-1, d)
            if hasattr(self._traj_ctx, "ensemble_moments") and len(xs):
                # the device reduction of the C-ABI (nyx_hip_ensemble_moments: moments_kernel.hip) - the 55 numbers a Rust host
                # would all-reduce; injected evaluators (the CPU tests' oracle stand-ins) have no such entry and take the numpy sums
                b = _abi.StateBatch(len(xs))
                b.set_rv(xs[:, :6])
                b.cr[:], b.cd[:], b.prop_mass_kg[:] = xs[:, 6], xs[:, 7], xs[:, 8]
                mom = self._traj_ctx.ensemble_moments(b, None, x0)
            else:
                xs = xs - x0
                mom = np.concatenate([[float(len(xs))], xs.sum(axis=0), (xs.T @ xs)[iu]])
        except Exception as e:  # noqa: BLE001 - re-raised on every rank below
            err = e
        self._sync_errors(err)
        if self._dist is not None and self._dist.get_world_size() > 1:
            mom = all_reduce_sum(self._dist, mom)
        n, sx = mom[0], mom[1:1 + d]
        if n < 1:   # no successful run anywhere: nothing to average
            return np.full(d, np.nan), np.full((d, d), np.nan)
        sxx = np.zeros((d, d))
        sxx[iu] = mom[1 + d:]
        sxx = sxx + np.triu(sxx, 1).T
        mean = sx / n
        cov = (sxx - n * np.outer(mean, mean)) / (n - 1.0) if n > 1 else np.full((d, d), np.nan)
        return mean + x0, cov

    # ---- reports (results.rs:86-245): one flat list, run after run, failed runs replaced by `value_if_run_failed`
    def _value(self, param: StateParameter, run: Run, rv: np.ndarray) -> np.ndarray:
        s = run.result.state
        return state_value(param, rv, self.mu_km3_s2, cr=s.cr, cd=s.cd, dry_mass_kg=s.dry_mass_kg, prop_mass_kg=s.prop_mass_kg,
                           extra_mass_kg=getattr(s, "extra_mass_kg", 0.0))

    def _sync_errors(self, err: Optional[BaseException]) -> None:
        """Sharded ensemble: a rank that fails BEFORE a collective would leave the others waiting in it for ever.  Every rank
        therefore reduces an error flag first and all of them raise - the failing rank its own exception, the others a
        RuntimeError naming the situation."""
        if self._dist is not None and self._dist.get_world_size() > 1:
            failed = all_reduce_sum(self._dist, np.array([1.0 if err is not None else 0.0]))[0]
            if err is None and failed > 0:
                raise RuntimeError("another rank failed while preparing this collective report; aborted on every rank")
        if err is not None:
            raise err

    def _gather_series(self, err: Optional[BaseException], head: np.ndarray, cols, n_rows: int, fill: float):
        """The common end of the array reports: `head[k]` (see `_fill_head`) and `cols[k]` (values[n_rows, len], or None for a
        failed run: a column of `fill`) of the local runs -> (values[n_rows, k_max, runs], len[runs], epoch0_ns[runs], ok[runs],
        k_max, bounds) over ALL the runs; slots past a run's len are NaN.  `err`: what the caller's preparation raised, re-raised
        on every rank (`_sync_errors`) before the first collective.  Sharded ensemble: the heads, then the rows are gathered in
        index order; `bounds` are the shards' positions (None when not sharded)."""
        self._sync_errors(err)
        bounds = None
        if self._dist is not None and self._dist.get_world_size() > 1:
            world = self._dist.get_world_size()
            bounds = [shard_bounds(len(self.runs), r, world) for r in range(world)]
            head = all_gather_rows(self._dist, head, bounds)
        k_max = int(head[:, 0].max()) if len(head) else 0
        local = np.full((len(cols), n_rows * k_max), np.nan)
        view = local.reshape(len(cols), n_rows, k_max)
        for k, col in enumerate(cols):
            if col is None:
                view[k] = fill
            else:
                view[k, :, :col.shape[1]] = col
        if bounds is not None and local.shape[1]:
            local = all_gather_rows(self._dist, local, bounds)
        values = np.ascontiguousarray(local.reshape(len(head), n_rows, k_max).transpose(1, 2, 0))
        return values, head[:, 0].astype(np.int32), np.ascontiguousarray(head[:, 1]).view(np.int64).copy(), head[:, 2] > 0, k_max, bounds

    def _report(self, param: StateParameter, states_of_run, value_if_run_failed: Optional[float], prepare=None) -> List[float]:
        """One flat list, run after run.  Sharded ensemble: every rank reports the runs it propagated (it holds their
        trajectories) and the pieces are gathered in rank order = index order (contiguous shards): a collective call.
        `prepare` (optional) runs first, inside the guarded section, and returns `states_of_run`."""
        report: List[float] = []
        err = None
        try:
            if prepare is not None:
                states_of_run = prepare()
            for run in self._local_runs():
                if not isinstance(run.result, PropResult):
                    if value_if_run_failed is not None:
                        report.append(float(value_if_run_failed))
                    continue
                rv = states_of_run(run)
                try:
                    report.extend(self._value(param, run, rv).ravel().tolist())
                except StateError:
                    # (the reference pushes the substitute once per state that cannot be evaluated)
                    if value_if_run_failed is not None:
                        report.extend([float(value_if_run_failed)] * len(rv))
        except Exception as e:  # noqa: BLE001 - re-raised on every rank by _sync_errors
            err = e
        self._sync_errors(err)
        if self._dist is not None and self._dist.get_world_size() > 1:
            report = all_gather_lists(self._dist, report)
        return report

    def _need_traj(self):
        if self._traj_batch is None:
            raise ValueError("these results carry no trajectories (with_traj=False)")

    def _every_batch(self, step_ns: int):
        """`Traj::every(step)` of all the runs of this process with one launch: a TrajBatch of the resampled states."""
        self._need_traj()
        tb = self._traj_batch
        last = np.array([tb.epoch_ns[max(min(int(tb.len[i]), tb.capacity) - 1, 0), i] for i in range(tb.n)])
        count = int(np.max(np.abs(last - tb.epoch_ns[0]) // abs(int(step_ns)))) + 1 if tb.n else 1
        return self._traj_ctx.traj_every(tb, int(step_ns), count) if tb.n else None   # (each rank resamples ITS shard on its device)

    def _states_between(self, run, step_ns: int, start_ns: int, end_ns: int) -> np.ndarray:
        """`Traj::every_between` of one run (traj.rs:153-162): its states [len, 6], one `traj_at` on a one-row batch."""
        self._need_traj()
        tb = self._traj_batch
        i = self._traj_rows[run.index]
        ep, _ = tb.trajectory(i)
        lo, hi = max(int(start_ns), int(ep.min())), min(int(end_ns), int(ep.max()))
        if hi < lo:
            return np.zeros((0, 6))
        q = lo + int(step_ns) * np.arange((hi - lo) // int(step_ns) + 1, dtype=np.int64)
        one = _abi.TrajBatch(1, max(len(ep), 1))
        one.len[0] = len(ep)
        one.epoch_ns[: len(ep), 0] = tb.epoch_ns[: len(ep), i]
        one.state[:, : len(ep), 0] = tb.state[:, : len(ep), i]
        states, status = self._traj_ctx.traj_at(one, q)
        bad = np.nonzero(_abi.interp_failed(status[:, 0]))[0]
        return states[: (bad[0] if len(bad) else len(q)), 0]

    def every_value_of(self, param: StateParameter, step_ns: int, value_if_run_failed: Optional[float] = None) -> List[float]:
        """results.rs:127-160: `param` of every run from the start to the end of its trajectory every `step_ns`."""
        def prepare():
            res = self._every_batch(step_ns)
            return lambda run: res.trajectory(self._traj_rows[run.index])[1]

        return self._report(param, None, value_if_run_failed, prepare=prepare)

    def every_value_of_between(self, param: StateParameter, step_ns: int, start_ns: int, end_ns: int,
                               value_if_run_failed: Optional[float] = None) -> List[float]:
        """results.rs:89-125: as above between max(start, first epoch) and min(end, last epoch) of each run
        (`Traj::every_between`, traj.rs:153-162; the series stops at the first epoch that cannot be interpolated)."""
        def states_of_run(run):
            return self._states_between(run, step_ns, start_ns, end_ns)

        return self._report(param, states_of_run, value_if_run_failed)

    def _composed(self, step: int, start_ns: Optional[int], end_ns: Optional[int], value):
        """The `composed` of a report for `_series`: `value(run, rv[len, 6], epochs[len])` -> values[n_rows, <= len] on the resampled
        states of every run - without a window ONE `traj_every` of all the runs of this process, with one a `traj_at` per run."""
        def composed(tb, rows):
            first = series_bounds(tb, start_ns, end_ns)[0]
            res = self._every_batch(step) if start_ns is None else None

            def column(run, row):
                rv = res.trajectory(row)[1] if start_ns is None else self._states_between(run, step, start_ns, end_ns)
                return value(run, rv, int(first[row]) + step * np.arange(len(rv), dtype=np.int64))

            return column, first

        return composed

    def _series(self, name: str, n_rows: int, fill: float, start_ns: Optional[int], end_ns: Optional[int], check, entry: str, fused, composed):
        """The one path of the array reports (`values_of`, `ric_dispersions`, `ground_tracks`, `station_views`, `eclipses`, `frame_values`, `link_views`), which
        describe their own part with three closures:
        `check()` raises what the report refuses, after the window check and before `_need_traj` (a check that has more to refuse after
        `_need_traj` calls it itself, as that of `ric_dispersions` does to keep its order of refusals);
        `fused(tb, rows)` serves an evaluator that has the fused `entry` with one launch over the batch `tb` (`rows`: those of the
        successful local runs), `composed(tb, rows)` any other by composition (`_composed`) - that is the definition, the device is
        tested against it; both return (column(run, row) -> values[n_rows, len] of one successful run, first epoch of every row of `tb`).
        -> what `_gather_series` returns.  A failed run is a column of `fill` with len 0.  Whatever the preparation raises is
        carried to `_gather_series`, which raises on every rank before the first collective."""
        runs = self._local_runs()
        head = np.zeros((len(runs), 3))                      # len, first epoch (bit pattern), run succeeded
        cols = [None] * len(runs)                            # values[n_rows, len] of every successful run
        err = None
        try:
            if (start_ns is None) != (end_ns is None):
                raise ValueError(f"{name}: a window needs both start_ns and end_ns")
            check()
            self._need_traj()
            ok = [k for k, run in enumerate(runs) if isinstance(run.result, PropResult)]
            rows = [self._traj_rows[runs[k].index] for k in ok]
            if ok:
                column, first = (fused if hasattr(self._traj_ctx, entry) else composed)(self._traj_batch, rows)
                for k, row in zip(ok, rows):
                    cols[k] = column(runs[k], row)
                    _fill_head(head, k, cols[k].shape[1], first[row])
        except Exception as e:  # noqa: BLE001 - re-raised on every rank by _sync_errors
            err = e
        return self._gather_series(err, head, cols, n_rows, fill)

    def values_of(self, params, step_ns: int, start_ns: Optional[int] = None, end_ns: Optional[int] = None,
                  value_if_run_failed: Optional[float] = None) -> "ValueSeries":
        """The array form of the list reports: `params` (a sequence of StateParameter) of every run every `step_ns`, from the
        start to the end of its trajectory, or between max(start, first epoch) and min(end, last epoch) when a window is given
        (`every_value_of` / `every_value_of_between`; sample 0 of a run is its `first_values_of`, a window [end, end] its
        `last_values_of`).  One ValueSeries for all of them, evaluated from ONE resampling.

        Orbit-derived parameters come fused from the device (`traj_values`: resampled, evaluated, only the values copied back);
        Cr, Cd and the masses are constants of a run and are filled in here; Isp / Thrust raise StateError.  A failed run is a
        column of `value_if_run_failed` (NaN when None) with len 0.  Sharded ensemble: a collective call, every rank reports
        the runs it propagated and the columns are gathered in index order.
        An evaluator without `traj_values` (the injected CPU evaluators of the tests) is served by `traj_every` / `traj_at` +
        `state_value`: that composition is the definition of the result, the device path is tested against it."""
        params = list(params)
        step = int(step_ns)
        orbit = [k for k, p in enumerate(params) if getattr(p, "name", None) in _abi.STATE_PARAM]

        def check():   # (no refusal of a non-positive step here: the list reports have none either)
            for p in params:
                if p in (StateParameter.Isp, StateParameter.Thrust) or not isinstance(p, StateParameter):
                    raise StateError(p)

        def fused(tb, rows):
            ask = [params[k] for k in orbit] or [StateParameter.X]   # (the lengths of the series come from the launch too)
            vals, length = self._traj_ctx.traj_values(tb, ask, step, start_ns, end_ns, mu_km3_s2=self.mu_km3_s2 if self.mu_km3_s2 > 0 else None)

            def column(run, row):
                got = vals[:len(orbit), :min(int(length[row]), vals.shape[1]), row]
                col = np.empty((len(params), got.shape[1]))
                for j, p in enumerate(params):   # Cr, Cd and the masses are constants of the run: any rv of the right length does
                    col[j] = got[orbit.index(j)] if j in orbit else self._value(p, run, np.zeros((got.shape[1], 6)))
                return col

            return column, series_bounds(tb, start_ns, end_ns)[0]

        def value(run, rv, ep):
            col = np.empty((len(params), len(rv)))
            for j, p in enumerate(params):
                col[j] = self._value(p, run, rv)
            return col

        fill = np.nan if value_if_run_failed is None else float(value_if_run_failed)
        values, length, epoch0, ok, _, _ = self._series("values_of", len(params), fill, start_ns, end_ns, check, "traj_values", fused,
                                                        self._composed(step, start_ns, end_ns, value))
        return ValueSeries(params, values, length, epoch0, step, ok)

    def _states_of_pair(self, row: int, ref, lo: int, hi: int, step: int):
        """(rx[len, 6], tx[len, 6], epochs[len]) of one run and the batch `ref` of one trajectory on their common grid: two
        `traj_at`, cut at the first epoch either cannot be interpolated at."""
        if hi < lo:
            return np.zeros((0, 6)), np.zeros((0, 6)), np.zeros(0, dtype=np.int64)
        tb = self._traj_batch
        q = lo + step * np.arange((hi - lo) // step + 1, dtype=np.int64)
        m = min(int(tb.len[row]), tb.capacity)
        one = _abi.TrajBatch(1, max(m, 1))
        one.len[0] = m
        one.epoch_ns[:m, 0] = tb.epoch_ns[:m, row]
        one.state[:, :m, 0] = tb.state[:, :m, row]
        a, sa = self._traj_ctx.traj_at(one, q)
        b, sb = self._traj_ctx.traj_at(ref, q)
        bad = np.nonzero(_abi.interp_failed(sa[:, 0]) | _abi.interp_failed(sb[:, 0]))[0]
        k = int(bad[0]) if len(bad) else len(q)
        return a[:k, 0], b[:k, 0], q[:k]

    def _ric_of_run(self, row: int, ref, lo: int, hi: int, step: int, frame_of, transport: bool, window: int) -> np.ndarray:
        """d[6, len] of one run against the nominal by composition: `_states_of_pair`, `ric_difference`, `smooth_ric`."""
        if hi < lo:
            return np.zeros((6, 0))
        a, b, _ = self._states_of_pair(row, ref, lo, hi, step)
        d = ric_difference(a, b, frame_of=frame_of, transport=transport)
        return (smooth_ric(d, window) if window >= 3 else d).T

    def ric_dispersions(self, nominal, step_ns: int, start_ns: Optional[int] = None, end_ns: Optional[int] = None, frame_of="reference",
                        transport: bool = True, smooth_window: int = 5) -> "RicSeries":
        """The dispersions of the ensemble around `nominal` (a Traj, or a TrajBatch of one trajectory) over time: the difference
        of every run to it in the radial / in-track / cross-track frame every `step_ns` over the overlap of the two spans
        (clamped to the window when given), with the count, mean and unbiased covariance of every sample - what
        `Traj::ric_diff_to_parquet` (traj.rs:407-600) computes for one pair, for all runs at once -> RicSeries.
        `frame_of="reference"`: the frame of the nominal ("run": of each run, the reference's `self.ric_difference(&other)`);
        `transport`: the rotation of that frame removed from the velocity differences; `smooth_window`: the reference's in-place
        median filter (it uses 5; 0 or 1: none).

        With a device evaluator one fused launch (`traj_ric_diff`: both trajectories resampled, differenced, filtered and
        summed on the device; 6 K doubles per run and 28 K sums copied back).  A failed run is a column of NaN with len 0, left out of
        the statistics.  Sharded ensemble: a collective call - every rank reports the runs it propagated, the columns are
        gathered in index order and the 28 K sums added with one all-reduce; every rank passes the same nominal.
        An evaluator without `traj_ric_diff` (the injected CPU evaluators of the tests) is served by `traj_at` +
        `ric_difference` + `smooth_ric` + numpy sums: that composition is the definition, the device path is tested against it."""
        step = int(step_ns)
        window = int(smooth_window)
        ref = mom = None
        made = []                                            # d[6, len] of the local runs, when they are composed here

        def check():
            nonlocal ref
            if frame_of not in FRAME_OF:
                raise ValueError(f"ric_dispersions: frame_of must be 'run' / 0 or 'reference' / 1, not {frame_of!r}")
            if window < 0 or window > _abi.RIC_MAX_WINDOW or (window and window % 2 == 0) or step <= 0:
                raise ValueError(f"ric_dispersions: a positive step and smooth_window 0 or odd up to {_abi.RIC_MAX_WINDOW}")
            self._need_traj()                                # (results without trajectories are refused before the nominal is looked at)
            ref = nominal._single() if hasattr(nominal, "_single") else nominal
            if ref.n != 1:
                raise ValueError("ric_dispersions: one nominal trajectory")

        def fused(tb, rows):
            nonlocal mom
            live = copy.copy(tb)                             # the same arrays; the rows of the failed runs emptied: no series, no share in the sums
            live.len = np.zeros_like(tb.len)
            live.len[rows] = tb.len[rows]
            vals, length, epoch0, mom = self._traj_ctx.traj_ric_diff(live, ref, step, start_ns, end_ns, frame_of=frame_of, transport=transport,
                                                                     smooth_window=window, moments=True)
            return (lambda run, row: vals[:, :min(int(length[row]), vals.shape[1]), row]), epoch0

        def composed(tb, rows):
            first, last = ric_bounds(tb, ref, start_ns, end_ns)

            def column(run, row):
                made.append(self._ric_of_run(row, ref, int(first[row]), int(last[row]), step, frame_of, bool(transport), window))
                return made[-1]

            return column, first

        values, length, epoch0, ok, k_max, bounds = self._series("ric_dispersions", 6, np.nan, start_ns, end_ns, check, "traj_ric_diff", fused, composed)
        if mom is None:
            mom = ric_moments(made, k_max)
        else:   # (the device sized its sums by the longest LOCAL series)
            mom = np.concatenate([mom[:k_max], np.zeros((max(k_max - len(mom), 0), _abi.RIC_MOMENTS))])
        if bounds is not None and k_max:
            mom = all_reduce_sum(self._dist, mom.ravel()).reshape(k_max, _abi.RIC_MOMENTS)
        count, mean, cov = ric_mean_cov(mom)
        return RicSeries(values, length, epoch0, step, ok, count, mean, cov, mom)

    def ground_tracks(self, frame, step_ns: int, params=GROUND_TRACK_DEFAULT, start_ns: Optional[int] = None,
                      end_ns: Optional[int] = None) -> "GroundTrackSeries":
        """The ground tracks of the ensemble: `params` (GroundTrackParameter members; by default the four fields of
        `Traj::to_groundtrack_parquet`, sc_traj.rs:131-155: geodetic latitude, longitude, height, |r|) of every run every
        `step_ns` in the body-fixed `frame` (an IAU-oriented frame of the runs' centre), from the start to the end of its
        trajectory or between max(start, first epoch) and min(end, last epoch) when a window is given -> GroundTrackSeries.

        With a device evaluator one fused launch per eight parameters (`traj_ground_track`: resampled, rotated at each sample's
        epoch, evaluated; only the values copied back).  A failed run is a column of NaN with len 0.  Sharded ensemble: a
        collective call, every rank reports the runs it propagated and the columns are gathered in index order.
        An evaluator without `traj_ground_track` (the injected CPU evaluators of the tests) is served by `traj_every` /
        `traj_at` + `groundtrack.ground_track_value`: that composition is the definition, the device path is tested against it."""
        params = list(params)
        step = int(step_ns)

        def check():
            if step <= 0:
                raise ValueError("ground_tracks: a positive step")
            for p in params:
                if not isinstance(p, GroundTrackParameter):
                    raise TypeError(f"{p!r} is not a GroundTrackParameter")
            if not params:
                raise ValueError("ground_tracks: at least one parameter")
            central = getattr(getattr(self._traj_ctx, "compiled", None), "central", None)
            check_frame(frame, central.naif_id if central is not None else None, params)

        def fused(tb, rows):
            vals, length = self._traj_ctx.traj_ground_track(tb, frame, params, step, start_ns, end_ns)
            return (lambda run, row: vals[:, :min(int(length[row]), vals.shape[1]), row]), series_bounds(tb, start_ns, end_ns)[0]

        def value(run, rv, ep):
            yf = to_body_fixed(rv, ep, frame)
            return np.stack([body_fixed_value(p, yf, frame.mean_equatorial_radius_km, frame.flattening) for p in params]).reshape(len(params), len(rv))

        values, length, epoch0, ok, _, _ = self._series("ground_tracks", len(params), np.nan, start_ns, end_ns, check, "traj_ground_track", fused,
                                                        self._composed(step, start_ns, end_ns, value))
        return GroundTrackSeries(params, values, length, epoch0, step, ok, frame)

    def station_views(self, stations, step_ns: int, params=AER_DEFAULT, start_ns: Optional[int] = None,
                      end_ns: Optional[int] = None) -> "AerSeries":
        """What every one of `stations` (GroundStation, all of one IAU-oriented frame of the runs' centre) sees of the ensemble:
        `params` (AerParameter members; by default azimuth, elevation, range and range rate, what
        `MeasurementType::compute_one_way` reads, od/msr/types.rs:102-117) of every run every `step_ns`, from the start to the
        end of its trajectory or between max(start, first epoch) and min(end, last epoch) when a window is given -> AerSeries.
        The geometry of `GroundStation::azimuth_elevation_of` only: no noise, no light time, no measurement update.

        With a device evaluator one fused launch per eight parameters and sixteen stations (`traj_aer`: resampled, rotated at
        each sample's epoch - once for all stations -, evaluated; only the values copied back).  A failed run is a column of NaN
        with len 0.  Sharded ensemble: a collective call, every rank reports the runs it propagated and the columns are gathered
        in index order.  An evaluator without `traj_aer` (the injected CPU evaluators of the tests) is served by `traj_every` /
        `traj_at` + `stations.aer_value`: that composition is the definition, the device path is tested against it."""
        stations, params = list(stations), list(params)
        step = int(step_ns)
        rows_out = len(stations) * len(params)               # the gather sees values[S * P, len] of every run

        def check():
            if step <= 0:
                raise ValueError("station_views: a positive step")
            for p in params:
                if not isinstance(p, AerParameter):
                    raise TypeError(f"{p!r} is not an AerParameter")
            if not params:
                raise ValueError("station_views: at least one parameter")
            central = getattr(getattr(self._traj_ctx, "compiled", None), "central", None)
            check_stations(stations, central.naif_id if central is not None else None)

        def fused(tb, rows):
            vals, length = self._traj_ctx.traj_aer(tb, stations, params, step, start_ns, end_ns)

            def column(run, row):
                m = min(int(length[row]), vals.shape[2])
                return vals[:, :, :m, row].reshape(rows_out, m)

            return column, series_bounds(tb, start_ns, end_ns)[0]

        def composed(tb, rows):
            consts = [station_consts(st) for st in stations]

            def value(run, rv, ep):
                yf = to_body_fixed(rv, ep, stations[0].frame)    # (the one frame of all of them: check_stations)
                return np.stack([sez_value(p, yf, c) for c in consts for p in params]).reshape(rows_out, len(rv))

            return self._composed(step, start_ns, end_ns, value)(tb, rows)

        values, length, epoch0, ok, k_max, _ = self._series("station_views", rows_out, np.nan, start_ns, end_ns, check, "traj_aer", fused, composed)
        return AerSeries(stations, params, values.reshape(len(stations), len(params), k_max, values.shape[2]), length, epoch0, step, ok)

    def eclipses(self, model, step_ns: int, params=ECLIPSE_DEFAULT, start_ns: Optional[int] = None, end_ns: Optional[int] = None) -> "EclipseSeries":
        """The eclipse history of the ensemble: `params` of the shadow `model` (eclipse.ShadowModel; an EclipseParameter, or a
        pair (per-body EclipseParameter, frame or index); by default the percentage hidden and the state, `ShadowModel::compute`,
        cosmic/eclipse.rs:69-83) of every run every `step_ns`, from the start to the end of its trajectory or between
        max(start, first epoch) and min(end, last epoch) when a window is given -> EclipseSeries.

        With a device evaluator one fused launch per eight parameters (`traj_eclipse`: resampled, the almanac evaluated at each
        sample's epoch, the disks overlapped; only the values copied back).  A failed run is a column of NaN with len 0.  Sharded
        ensemble: a collective call.  An evaluator without `traj_eclipse` (the injected CPU evaluators of the tests) is served by
        `traj_every` / `traj_at` + `eclipse.eclipse_value`: that composition is the definition, the device path is tested against it."""
        params = list(params)
        step = int(step_ns)
        compiled = getattr(self._traj_ctx, "compiled", None)
        almanac, central = getattr(compiled, "almanac", None), getattr(compiled, "central", None)
        pairs = [p if isinstance(p, tuple) else (p, None) for p in params]

        def check():
            if step <= 0:
                raise ValueError("eclipses: a positive step")
            if not params:
                raise ValueError("eclipses: at least one parameter")
            if almanac is None or central is None:
                raise ValueError("eclipses: the evaluator does not know the almanac and the central frame of the runs")
            check_shadow_model(model, almanac, central)

        def fused(tb, rows):
            vals, length = self._traj_ctx.traj_eclipse(tb, model, params, step, start_ns, end_ns)
            return (lambda run, row: vals[:, :min(int(length[row]), vals.shape[1]), row]), series_bounds(tb, start_ns, end_ns)[0]

        def value(run, rv, ep):
            col = np.stack([eclipse_value(p, rv, ep, model, almanac, central, body=b) for p, b in pairs]).reshape(len(params), len(rv))
            bad = np.nonzero(np.isnan(col).any(axis=0))[0]   # (a sample outside the ephemerides ends the series)
            return col[:, :int(bad[0])] if len(bad) else col

        values, length, epoch0, ok, _, _ = self._series("eclipses", len(params), np.nan, start_ns, end_ns, check, "traj_eclipse", fused,
                                                        self._composed(step, start_ns, end_ns, value))
        return EclipseSeries(model, params, values, length, epoch0, step, ok)

    def frame_values(self, target, params, step_ns: int, start_ns: Optional[int] = None, end_ns: Optional[int] = None) -> "FrameSeries":
        """The ensemble seen from another body: `params` (FrameParameter members, or the orbit-derived StateParameter of the same
        name) of every run about `target` - a Frame of the runs' orientation with another ephemeris id and its own mu - every
        `step_ns`, from the start to the end of its trajectory or between max(start, first epoch) and min(end, last epoch) when a
        window is given -> FrameSeries.  `Traj::to_frame` (sc_traj.rs:88-129) then the elements and the B-plane (cosmic/bplane.rs)
        about the target.

        With a device evaluator one fused launch per eight parameters (`traj_frame_values`: resampled, the almanac evaluated at each
        sample's epoch, the state translated, the parameters evaluated; only the values copied back).  A failed run is a column of
        NaN with len 0; a sample outside the ephemerides ends a series, one that is not hyperbolic has NaN B-plane values and does
        not.  Sharded ensemble: a collective call.  An evaluator without `traj_frame_values` (the injected CPU evaluators of the
        tests) is served by `traj_every` / `traj_at` + `frames.frame_value`: that composition is the definition, the device path is
        tested against it."""
        params = list(params)
        step = int(step_ns)
        compiled = getattr(self._traj_ctx, "compiled", None)
        almanac, central = getattr(compiled, "almanac", None), getattr(compiled, "central", None)
        codes = []

        def check():
            if step <= 0:
                raise ValueError("frame_values: a positive step")
            if not params:
                raise ValueError("frame_values: at least one parameter")
            codes[:] = [frame_param(p) for p in params]
            if almanac is None or central is None:
                raise ValueError("frame_values: the evaluator does not know the almanac and the central frame of the runs")
            check_target(target, almanac, central)

        def fused(tb, rows):
            vals, length = self._traj_ctx.traj_frame_values(tb, target, codes, step, start_ns, end_ns)
            return (lambda run, row: vals[:, :min(int(length[row]), vals.shape[1]), row]), series_bounds(tb, start_ns, end_ns)[0]

        def value(run, rv, ep):
            moved = np.asarray(frame_value(FrameParameter.X, rv, ep, target, almanac, central)).reshape(len(rv))
            col = np.stack([frame_value(p, rv, ep, target, almanac, central) for p in codes]).reshape(len(codes), len(rv))
            bad = np.nonzero(np.isnan(moved))[0]             # (a sample outside the ephemerides ends the series; a NaN B-plane value does not)
            return col[:, :int(bad[0])] if len(bad) else col

        values, length, epoch0, ok, _, _ = self._series("frame_values", len(params), np.nan, start_ns, end_ns, check, "traj_frame_values", fused,
                                                        self._composed(step, start_ns, end_ns, value))
        return FrameSeries(target, codes, values, length, epoch0, step, ok)

    def link_views(self, transmitter, step_ns: int, params=LINK_DEFAULT, bodies=None, start_ns: Optional[int] = None,
                   end_ns: Optional[int] = None) -> "LinkSeries":
        """The ensemble seen from another spacecraft: `params` (a LinkParameter, or a pair (per-body LinkParameter, frame or index);
        by default range, range rate and visibility) of the link from `transmitter` (a Traj, or a TrajBatch of one trajectory) to
        every run every `step_ns` over the overlap of the two spans (clamped to the window when given) -> LinkSeries.  `bodies`:
        the Frames that can block the line; None: the runs' centre with its mean equatorial radius, what the reference's
        `InterlinkTxSpacecraft::measure_instantaneous` (od/interlink/trk_device.rs) obstructs with.  The instantaneous geometry
        only: no noise, no light time, no integration-time average.

        With a device evaluator one fused launch per eight parameters (`traj_link`: both trajectories resampled, the almanac
        evaluated at each sample's epoch, the SIGHT test; only the values copied back).  A failed run is a column of NaN with len 0.
        Sharded ensemble: a collective call, every rank passes the same transmitter.  An evaluator without `traj_link` (the injected
        CPU evaluators of the tests) is served by `traj_at` + `links.link_value`: that composition is the definition, the device path
        is tested against it."""
        params = list(params)
        step = int(step_ns)
        compiled = getattr(self._traj_ctx, "compiled", None)
        almanac, central = getattr(compiled, "almanac", None), getattr(compiled, "central", None)
        ref = None
        who, pairs = [], []

        def check():
            nonlocal ref
            if step <= 0:
                raise ValueError("link_views: a positive step")
            if not params:
                raise ValueError("link_views: at least one parameter")
            if central is None:
                raise ValueError("link_views: the evaluator does not know the central frame of the runs")
            who[:] = default_bodies(central) if bodies is None else list(bodies)
            check_link_bodies(who, almanac, central)
            pairs[:] = [link_param(p, who) for p in params]
            self._need_traj()                                # (results without trajectories are refused before the transmitter is looked at)
            ref = transmitter._single() if hasattr(transmitter, "_single") else transmitter
            if ref.n != 1:
                raise ValueError("link_views: one transmitter trajectory")

        def fused(tb, rows):
            live = copy.copy(tb)                             # the same arrays; the rows of the failed runs emptied: no series
            live.len = np.zeros_like(tb.len)
            live.len[rows] = tb.len[rows]
            vals, length, epoch0 = self._traj_ctx.traj_link(live, ref, params, step, start_ns, end_ns, bodies=who)
            return (lambda run, row: vals[:, :min(int(length[row]), vals.shape[1]), row]), epoch0

        def composed(tb, rows):
            first, last = ric_bounds(tb, ref, start_ns, end_ns)

            def column(run, row):
                rx, tx, ep = self._states_of_pair(row, ref, int(first[row]), int(last[row]), step)
                col = np.stack([link_value(p, rx, tx, ep, who, almanac, central, body=b) for p, b in pairs]).reshape(len(pairs), len(ep))
                bad = np.nonzero(outside_ephemerides(ep, who, almanac, central))[0]   # (a sample outside the ephemerides ends the series)
                return col[:, :int(bad[0])] if len(bad) else col

            return column, first

        values, length, epoch0, ok, _, _ = self._series("link_views", len(params), np.nan, start_ns, end_ns, check, "traj_link", fused, composed)
        return LinkSeries(list(who), params, values, length, epoch0, step, ok)

    def series_stats(self, report: str, *args, probs=(), **kwargs) -> "series_statistics.SeriesStats":
        """The statistics over the runs of one of the array reports (`report`: "values_of", "ric_dispersions", "ground_tracks",
        "station_views", "eclipses", "frame_values" or "link_views", with the arguments of that report): per row and sample the
        runs that hold it, the extremes and which runs they are, the sums behind mean and sigma and the exact quantiles `probs` ->
        stats.SeriesStats (include/nyx_hip_stats.h; nyx_amd/stats.py is the definition).  A failed run is left out.

        With a device evaluator, an ensemble that is not sharded and rows that all come from the device (no Cr, Cd or mass column
        of `values_of`) the report and the reduction run back to back on the device (`nyx_hip_traj_series_stats`) and only the
        statistics are copied back.  Otherwise - the injected CPU evaluators of the tests, a sharded ensemble on every rank - the
        named report as it is, then `stats.series_stats` on its values: that composition is the definition, the device path is
        tested against it.  Quantiles do not all-reduce: a distributed selection is out of scope."""
        if report not in SERIES_REPORTS:
            raise ValueError(f"series_stats: report must be one of {sorted(SERIES_REPORTS)}, not {report!r}")
        probs = tuple(float(p) for p in series_statistics.check_probs(probs))
        entry = SERIES_REPORTS[report]
        ctx = self._traj_ctx
        sharded = self._dist is not None and self._dist.get_world_size() > 1
        device_rows = report != "values_of" or all(getattr(p, "name", None) in _abi.STATE_PARAM for p in (args[0] if args else kwargs.get("params", ())))
        tap = None
        if hasattr(ctx, "series_stats") and hasattr(ctx, entry) and not sharded and device_rows and self._traj_batch is not None:
            status = np.ones(self._traj_batch.n, dtype=np.int32)
            status[[self._traj_rows[r.index] for r in self.runs if isinstance(r.result, PropResult)]] = 0
            tap = _StatsTap(ctx, entry, series_statistics.Request(probs, status))
            self._traj_ctx = tap
        try:
            series = getattr(self, report)(*args, **kwargs)
        finally:
            self._traj_ctx = ctx
        if report == "station_views":
            rows = [(st, p) for st in series.stations for p in series.params]
        else:
            rows = list(series.params) if hasattr(series, "params") else list(RIC_ROWS)
        if tap is not None and tap.stats is not None:
            live = status == 0
            k_max = int(np.minimum(tap.length[live], tap.stats.shape[-2]).max()) if live.any() else 0
            got = tap.stats.reshape(len(rows), tap.stats.shape[-2], tap.stats.shape[-1])[:, :k_max]
            first = tap.epoch0[live & (tap.length > 0)]
        else:
            values = series.values.reshape(len(rows), -1, series.values.shape[-1])
            got = series_statistics.series_stats(values, series.len, probs, status=(~np.asarray(series.ok)).astype(np.int32))
            first = series.epoch0_ns[np.asarray(series.ok) & (series.len > 0)]
        same = len(first) > 0 and bool((first == first[0]).all())
        return series_statistics.SeriesStats(got, rows, probs, step_ns=series.step_ns, epoch0_ns=int(first[0]) if same else None)

    def first_values_of(self, param: StateParameter, value_if_run_failed: Optional[float] = None) -> List[float]:
        """results.rs:162-190."""
        return self._report(param, None, value_if_run_failed,
                            prepare=lambda: (self._need_traj(), lambda run: np.asarray(run.result.traj.first())[None, :])[1])

    def last_values_of(self, param: StateParameter, value_if_run_failed: Optional[float] = None) -> List[float]:
        """results.rs:192-220."""
        return self._report(param, None, value_if_run_failed,
                            prepare=lambda: (self._need_traj(), lambda run: np.asarray(run.result.traj.last())[None, :])[1])

    def dispersion_values_of(self, param: StateParameter) -> List[float]:
        """results.rs:222-239: the applied dispersion of `param` for every run; StateError if it was not dispersed."""
        report = []
        for run in self.runs:
            for dparam, val in run.dispersed_state.actual_dispersions:
                if dparam == param:
                    report.append(val)
                    break
            else:
                raise StateError(param)
        return report


def _vec9(sc) -> np.ndarray:
    return np.concatenate([np.asarray(sc.rv, dtype=np.float64), [float(sc.cr), float(sc.cd), float(sc.prop_mass_kg)]])


def shard_bounds(n: int, rank: int, world: int):
    """Contiguous index shard [lo, hi) of rank `rank` (index-stable => resume/skip semantics carry over)."""
    base, rem = divmod(n, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


@dataclass
class MonteCarlo:
    """montecarlo.rs:44-75."""

    random_state: MvnSpacecraft
    seed: Optional[int] = None
    scenario: str = "MonteCarlo"
    nominal_state: Optional[Spacecraft] = None   # (carried for the reports' headers in the reference, montecarlo.rs:49-51)
    # injectable for the CPU tests (gloo): (batch, end_epoch_ns) -> (out batch, stats); default = the GPU context
    propagate_fn: Optional[Callable] = field(default=None, repr=False)

    def generate_states(self, skip: int, num_runs: int, seed: Optional[int] = None):
        """montecarlo.rs:277-296: one stream, samples drawn sequentially, first `skip` discarded."""
        use = self.seed if seed is None else seed
        # Pcg64Mcg::new(seed) (montecarlo.rs:284-287); without a seed the reference takes one from the OS
        rng = Pcg64Mcg(use if use is not None else int.from_bytes(os.urandom(16), "little"))
        t = self.random_state.template
        base = np.concatenate([np.asarray(t.rv, dtype=np.float64), [t.cr, t.cd, t.prop_mass_kg]])
        out = []
        for index in range(skip + num_runs):
            v = self.random_state.sample_vector(rng)
            if index < skip:
                continue
            x = base + v
            s = DispersedState(**{f: v for f, v in t.__dict__.items() if f != "actual_dispersions"})
            s.rv, s.cr, s.cd, s.prop_mass_kg = x[:6].copy(), float(x[6]), float(x[7]), float(x[8])
            # template.value(param) - state.value(param) for every dispersed component (multivariate.rs:320-325)
            mu = float(t.frame.mu_km3_s2)

            def val(sc, p):
                return float(state_value(p, np.asarray(sc.rv, dtype=np.float64), mu, cr=sc.cr, cd=sc.cd, dry_mass_kg=sc.dry_mass_kg,
                                         prop_mass_kg=sc.prop_mass_kg, extra_mass_kg=sc.extra_mass_kg))

            s.actual_dispersions = [(d.param, val(t, d.param) - val(s, d.param)) for d in self.random_state.dispersions]
            out.append((index - skip, s))   # `.skip(skip).take(num_runs).enumerate()`: a resumed run counts from 0 again (montecarlo.rs:290-295)
        return out

    def run_until_epoch(self, prop: Propagator, almanac: Almanac, end_epoch_ns: int, num_runs: int, with_traj: bool = True,
                        capacity: int = 4096) -> Results:
        return self.resume_run_until_epoch(prop, almanac, 0, end_epoch_ns, num_runs, with_traj=with_traj, capacity=capacity)

    def resume_run_until_epoch(self, prop: Propagator, almanac: Almanac, skip: int, end_epoch_ns: int, num_runs: int,
                               dist=None, with_traj: bool = True, capacity: int = 4096) -> Results:
        """montecarlo.rs:208-273: every run is `until_epoch_with_traj` (:236-239), so each PropResult carries its
        trajectory - recorded on the device by the propagation kernel, `capacity` accepted steps per run (doubled and
        re-run if a run needs more).  `with_traj=False` skips the dense output.  With `dist` (an initialised
        torch.distributed module) the runs are sharded by contiguous index range over the ranks and every rank returns the
        complete, index-sorted Results; trajectories stay on the rank that propagated them."""
        t_epoch = int(self.random_state.template.epoch_ns)

        def run(ctx, batch):
            if not with_traj:
                return ctx.propagate_until_epoch(batch, int(end_epoch_ns))
            cap = int(capacity)
            while True:
                out, st, traj = ctx.propagate_with_traj(batch, int(end_epoch_ns) - t_epoch, cap)
                need = int(traj.len.max()) if traj.n else 0
                if need <= cap:
                    return out, st, traj, ctx
                cap = max(2 * cap, need)

        return self._run(prop, almanac, skip, num_runs, dist, run, int(end_epoch_ns))

    def run_until_nth_event(self, prop: Propagator, almanac: Almanac, max_duration_ns: int, event, trigger: int, num_runs: int) -> Results:
        """montecarlo.rs:93-110."""
        return self.resume_run_until_nth_event(prop, almanac, 0, max_duration_ns, event, trigger, num_runs)

    def resume_run_until_nth_event(self, prop: Propagator, almanac: Almanac, skip: int, max_duration_ns: int, event, trigger: int,
                                   num_runs: int, dist=None, capacity: int = 4096) -> Results:
        """montecarlo.rs:115-186: every run stops at the `trigger`-th occurrence of `event` (or fails with NthEventError)."""

        def run(ctx, batch):
            out, st, traj, _ = ctx.propagate_until_event(batch, int(max_duration_ns), event, trigger, capacity)
            return out, st, traj, ctx

        return self._run(prop, almanac, skip, num_runs, dist, run, ("event", int(max_duration_ns), event, trigger))

    def _run(self, prop, almanac, skip, num_runs, dist, run, fn_arg) -> Results:
        from .propagator import PropagationError, pack_spacecraft

        rank, world = (dist.get_rank(), dist.get_world_size()) if dist is not None else (0, 1)
        seed = self.seed
        if world > 1 and seed is None:
            # every rank regenerates the whole stream and keeps its shard: without a seed they must still draw the SAME one
            seed = broadcast_seed(dist, None)
        states = self.generate_states(skip, num_runs, seed if seed is not None else None)
        lo, hi = shard_bounds(len(states), rank, world)
        mine = states[lo:hi]
        batch = pack_spacecraft([s for _, s in mine], False)
        # (out, stats) or (out, stats, TrajBatch, evaluator of trajectories: anything with traj_at / traj_every)
        got = self.propagate_fn(batch, fn_arg) if self.propagate_fn is not None else \
            run(prop._context(almanac, self.random_state.template.frame, False), batch)
        out, st = got[0], got[1]
        traj_batch, traj_ctx = (got[2], got[3]) if len(got) == 4 else (None, None)
        payload = np.concatenate([out.rv(), out.cr[:, None], out.cd[:, None], out.prop_mass_kg[:, None],
                                  np.ascontiguousarray(out.epoch_ns, dtype=np.int64).view(np.float64)[:, None],  # bit pattern: ns past J2000 exceed 2^53
                                  st.status[:, None].astype(np.float64)], axis=1)
        if dist is not None and world > 1:
            payload = all_gather_rows(dist, payload, [shard_bounds(len(states), r, world) for r in range(world)])
        runs = []
        for k, (index, s) in enumerate(states):
            row = payload[k]
            status = int(row[10])
            if status == _abi.OK:
                r = Spacecraft(**{f: v for f, v in s.__dict__.items() if f != "actual_dispersions"})
                r.rv, r.cr, r.cd, r.prop_mass_kg, r.epoch_ns = row[:6].copy(), float(row[6]), float(row[7]), float(row[8]), int(row[9:10].view(np.int64)[0])
                src = (traj_ctx, traj_batch, k - lo) if (traj_batch is not None and lo <= k < hi) else None
                runs.append(Run(index, s, PropResult(r, src)))
            else:
                runs.append(Run(index, s, PropagationError(status, index)))
        rows = {index: k - lo for k, (index, _) in enumerate(states) if lo <= k < hi} if traj_batch is not None else {}
        runs.sort(key=lambda r: r.index)  # par_sort_by_key(index), montecarlo.rs:267
        # every rank holds every final state; trajectories (and hence the reports' raw material) stay on the rank that
        # propagated them: Results gathers the report pieces / reduces the moments over `dist` (index order = rank order,
        # runs being sorted by index and the shards contiguous)
        sharded = dist is not None and world > 1
        return Results(runs, self.scenario, float(self.random_state.template.frame.mu_km3_s2), traj_ctx, traj_batch, rows,
                       dist if sharded else None, (lo, hi) if sharded else None)


def _coll_device(dist):
    import torch

    return torch.device("cuda", torch.cuda.current_device()) if dist.get_backend() == "nccl" else torch.device("cpu")


def all_reduce_sum(dist, v: np.ndarray) -> np.ndarray:
    """One all-reduce (sum) of a small f64 vector: the ensemble moments (RCCL over xGMI on GPUs; latency-bound at 55 doubles)."""
    import torch

    t = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to(_coll_device(dist))
    dist.all_reduce(t, op=dist.ReduceOp.SUM)
    return t.cpu().numpy()


def broadcast_seed(dist, seed: Optional[int]) -> int:
    """A 128-bit seed agreed by all ranks: rank 0's (drawn from the OS when None, as the reference does), as four int32-safe
    limbs in one int64 tensor."""
    import torch

    if dist.get_rank() == 0:
        seed = int.from_bytes(os.urandom(16), "little") if seed is None else int(seed)
    limbs = [((seed or 0) >> (32 * k)) & 0xFFFFFFFF for k in range(4)]
    t = torch.tensor(limbs, dtype=torch.int64, device=_coll_device(dist))
    dist.broadcast(t, src=0)
    return sum(int(x) << (32 * k) for k, x in enumerate(t.cpu().tolist()))


def all_gather_lists(dist, local: List[float]) -> List[float]:
    """Ragged all-gather of per-rank report pieces, concatenated in rank order: lengths first, then one padded all-gather."""
    import torch

    dev = _coll_device(dist)
    world = dist.get_world_size()
    n = torch.tensor([len(local)], dtype=torch.int64, device=dev)
    lens = [torch.zeros_like(n) for _ in range(world)]
    dist.all_gather(lens, n)
    lens = [int(x.item()) for x in lens]
    buf = torch.zeros(max(max(lens), 1), dtype=torch.float64, device=dev)
    if local:
        buf[: len(local)] = torch.tensor(local, dtype=torch.float64).to(dev)
    parts = [torch.empty_like(buf) for _ in range(world)]
    dist.all_gather(parts, buf)
    out: List[float] = []
    for r in range(world):
        out.extend(parts[r][: lens[r]].cpu().tolist())
    return out


def all_gather_rows(dist, local: np.ndarray, bounds) -> np.ndarray:
    """One all-gather of the per-rank result rows (ragged shards are padded to the largest)."""
    import torch

    world = dist.get_world_size()
    width = local.shape[1]
    nmax = max(hi - lo for lo, hi in bounds)
    backend = dist.get_backend()
    dev = torch.device("cuda", torch.cuda.current_device()) if backend == "nccl" else torch.device("cpu")
    buf = torch.zeros((nmax, width), dtype=torch.float64, device=dev)
    buf[: local.shape[0]] = torch.from_numpy(np.ascontiguousarray(local)).to(dev)
    parts = [torch.empty_like(buf) for _ in range(world)]
    dist.all_gather(parts, buf)
    return np.concatenate([parts[r][: hi - lo].cpu().numpy() for r, (lo, hi) in enumerate(bounds)], axis=0)
