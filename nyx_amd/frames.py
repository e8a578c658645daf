"""Encounters: an ensemble seen from another body - the state translated to another centre, its elements and its B-plane there.

Host-side definition of what `Traj::to_frame` (md/trajectory/sc_traj.rs:88-129: `almanac.transform_to(state.orbit, new_frame, None)`
for every state) computes between two frames of ONE orientation - a translation by the state of one centre relative to the other -
followed by a parameter evaluation about the new centre: the orbit-derived `StateParameter`s with the target's mu, and the B-plane of
the approach (cosmic/bplane.rs:55-136, 195-219).  The device kernel (csrc/frame_kernel.hip) is tested against this module, which
restates the oracle's `frame_shift` (oracle/nyx_oracle.c:143-161; the chain and `cheby_eval_pv` are chains.py's) OPERATION FOR
OPERATION - one rounding per operation - so that positions agree with the oracle bit for bit (tests/test_frame_host.py).

    body   = sum_k sign_k * (p_k, pv_k)                  the target's chain, in chain order, from zero
    rv'    = rv - body                                   no aberration, no light time (the reference passes None too)
    0..18  = params.state_value(rv', mu of the target)   the codes of nyx_hip_state_param
    C3     = vmag vmag - 2 mu / rmag,  VInfinity = sqrt(C3),  BdotT / BdotR = params.bplane_of_state,  BAngle = atan2(BdotR, BdotT) in degrees,
    BMagnitude = sqrt(BdotT^2 + BdotR^2)

Where ecc <= 1 the B-plane codes and VInfinity are NaN (`BPlane::new`: NotHyperbolic) and a series continues; an epoch outside a
segment of the target's chain gives a row of NaN (the device series ends there).  The reference's `BLTOF` has no code: in its
formula B . s^ is zero analytically, what is left is rounding noise.
"""
from __future__ import annotations

import enum
import math

import numpy as np

from .chains import MAX_CHAIN, body_chain, chain_state, checked_chain, cheby_state  # noqa: F401  (re-exported)
from .groundtrack import _TO_DEG, _libm, _ns_to_seconds
from .params import StateParameter, bplane_of_state, state_value


class FrameParameter(enum.IntEnum):
    """enum nyx_hip_frame_param (include/nyx_hip_frame.h): never renumber.  0 .. 18 are nyx_hip_state_param."""

    X = 0
    Y = 1
    Z = 2
    VX = 3
    VY = 4
    VZ = 5
    Rmag = 6
    Vmag = 7
    Hmag = 8
    Energy = 9
    SemiMajorAxis = 10
    Eccentricity = 11
    Inclination = 12
    RAAN = 13
    AoP = 14
    TrueAnomaly = 15
    Period = 16
    ApoapsisRadius = 17
    PeriapsisRadius = 18
    C3 = 19
    BdotT = 20
    BdotR = 21
    BAngle = 22            # deg, (-180, 180]
    BMagnitude = 23
    VInfinity = 24


HYPERBOLA_ONLY = frozenset({FrameParameter.BdotT, FrameParameter.BdotR, FrameParameter.BAngle, FrameParameter.BMagnitude, FrameParameter.VInfinity})
_atan2 = _libm(math.atan2, 2)


def frame_param(param) -> FrameParameter:
    """A FrameParameter from itself, its code, or the orbit-derived StateParameter of the same name."""
    if isinstance(param, FrameParameter):
        return param
    if isinstance(param, StateParameter):
        if param.name not in FrameParameter.__members__:
            raise TypeError(f"{param!r} is not a parameter of the encounter report")
        return FrameParameter[param.name]
    if isinstance(param, (int, np.integer)) and not isinstance(param, bool):
        return FrameParameter(int(param))
    raise TypeError(f"{param!r} is not a FrameParameter")


def check_target(target, almanac, central):
    """The chain of `target` w.r.t. `central` in `almanac`, refusing what `check_frame_series` (csrc/series_host.h) refuses: KeyError
    from `eclipse.body_chain` for a body the almanac cannot reach, ValueError for the rest."""
    chain = checked_chain(body_chain(target.naif_id, almanac, central), almanac, "encounter target: the frame")
    mu = float(target.mu_km3_s2)
    if not (math.isfinite(mu) and mu > 0.0):
        raise ValueError("encounter target: the frame needs a finite mu > 0")
    return chain


def body_state(naif_id: int, epoch_ns, almanac, central):
    """`frame_shift` of the oracle without the state: (r[..., 3], v[..., 3]) of a body w.r.t. `central`, the signed sum over its
    chain, in chain order, from zero."""
    return chain_state(body_chain(naif_id, almanac, central), _ns_to_seconds(epoch_ns), almanac)[:2]


def to_frame(rv, epoch_ns, target, almanac, central) -> np.ndarray:
    """`rv` ([..., 6], km and km/s, about `central`) at `epoch_ns` (broadcast) about `target`, a Frame of the same orientation:
    rv - body_state(target), component by component (`frame_shift` with dir = -1).  `target == central` is the identity; an epoch
    outside a segment of the chain gives a row of NaN."""
    rv = np.asarray(rv, dtype=np.float64)
    if not body_chain(target.naif_id, almanac, central):
        return rv.copy()
    epoch = np.broadcast_to(np.asarray(epoch_ns, dtype=np.int64), rv.shape[:-1])
    r, v = body_state(target.naif_id, epoch, almanac, central)
    return rv - np.concatenate([r, v], axis=-1)


def state_frame_value(param, rv, mu_km3_s2: float) -> np.ndarray:
    """Value of `param` (FrameParameter) for every row of a state `rv` ([..., 6]) about a centre of `mu_km3_s2`."""
    param = frame_param(param)
    rv = np.asarray(rv, dtype=np.float64)
    mu = float(mu_km3_s2)
    if param <= FrameParameter.PeriapsisRadius:
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.asarray(state_value(StateParameter[param.name], rv, mu), dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        rmag = state_value(StateParameter.Rmag, rv, mu)
        vmag = state_value(StateParameter.Vmag, rv, mu)
        c3 = vmag * vmag - 2.0 * mu / rmag
        if param is FrameParameter.C3:
            return c3
        ecc = state_value(StateParameter.Eccentricity, rv, mu)
        if param is FrameParameter.VInfinity:
            return np.where(ecc > 1.0, np.sqrt(c3), np.nan)
        bt, br = bplane_of_state(rv, mu)
        if param is FrameParameter.BdotT:
            return bt
        if param is FrameParameter.BdotR:
            return br
        if param is FrameParameter.BMagnitude:
            return np.sqrt(bt * bt + br * br)
        a = _atan2(br, bt) * _TO_DEG
        return np.where(a == -180.0, 180.0, a)


def frame_value(param, rv, epoch_ns, target, almanac, central) -> np.ndarray:
    """Value of `param` (FrameParameter) for every row of `rv` ([..., 6], km and km/s, about `central`) at `epoch_ns` (broadcast), seen
    from `target` (a Frame of the same orientation, with its own mu).  The per-sample definition the device kernel is tested against."""
    check_target(target, almanac, central)
    return state_frame_value(param, to_frame(rv, epoch_ns, target, almanac, central), float(target.mu_km3_s2))
