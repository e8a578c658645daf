"""Eclipses: how much of the light source a spacecraft sees, and which body hides it.

Host-side definition of what `ShadowModel::compute` (cosmic/eclipse.rs:69-83) computes through anise's
`Almanac::solar_eclipsing`: the apparent disk of the light source, the apparent disk of every shadow body, the share of the first
that the second hides, the body with the largest share (strict >, first wins).  The device kernel (csrc/eclipse_kernel.hip) is
tested against this module, which restates the oracle's `occultation_pct` (oracle/nyx_oracle.c; `body_position` / `cheby_eval` are
chains.py's) OPERATION FOR OPERATION - sums of three left to right, `norm3` as sqrt(x x + y y + z z), one rounding per
operation, asin / acos of the C library element by element - so that it agrees with the oracle bit for bit
(tests/test_eclipse_host.py).

    r_eb = r - p_body,  r_ls = p_sun - r                 no aberration, no light time (the reference passes None too)
    ls_p = R_s >= |r_ls| ? R_s : asin(R_s / |r_ls|)      fo_p likewise: THE QUIRK - nearer than the radius, the radius in km -
    d_p  = acos(-(r_ls . r_eb) / (|r_eb| |r_ls|))        is kept, and the degree-valued parameters report what the formula used
    lit (d_p - ls_p > fo_p) 0;  umbra (fo_p > d_p + ls_p) 100;  penumbra: the lens of two disks;  else annular 100 fo_p^2 / ls_p^2

Positions are signed sums of the almanac's Chebyshev segments along a body's chain, in chain order (chains.py).  An epoch outside
a segment gives NaN for that sample (the device series ends there).
"""
from __future__ import annotations

import enum
import math
from dataclasses import dataclass, field
from typing import List

import numpy as np

from .chains import MAX_CHAIN, body_chain, chain_state, checked_chain, cheby_position  # noqa: F401  (re-exported)
from .groundtrack import _TO_DEG, _libm, _ns_to_seconds


class EclipseParameter(enum.IntEnum):
    """enum nyx_hip_ecl_param (include/nyx_hip_eclipse.h): never renumber."""

    # of the whole shadow model
    Occultation = 0          # percent, 0 .. 100
    Illumination = 1         # |percentage / 100 - 1|, the k of SolarPressure::eom
    State = 2                # 0 lit, 1 partial (annular included), 2 umbra
    EclipsingBody = 3        # index into model.shadow_bodies of the winner, -1 when the percentage is 0
    SunRange = 4             # km
    SunApparentRadius = 5    # deg
    # of ONE body
    BodyOccultation = 6      # percent
    BodyApparentRadius = 7   # deg
    BodySeparation = 8       # deg: light-source centre to body centre as seen from the spacecraft
    BodyPenumbraMargin = 9   # deg: d_p - ls_p - fo_p, > 0 fully lit
    BodyUmbraMargin = 10     # deg: fo_p - d_p - ls_p, > 0 in the umbra


PER_BODY = frozenset(p for p in EclipseParameter if p >= EclipseParameter.BodyOccultation)
DEFAULT_PARAMS = (EclipseParameter.Occultation, EclipseParameter.State)
MAX_BODIES = 8


@dataclass
class ShadowModel:
    """cosmic/eclipse.rs:36-66: the light source and the bodies that can hide it, as Frames (NAIF id, mean radius)."""

    light_source: object
    shadow_bodies: List[object] = field(default_factory=list)

    @classmethod
    def cislunar(cls, almanac) -> "ShadowModel":
        """`ShadowModel::cislunar`: the Sun hidden by the Earth and the Moon."""
        from .propagator import EARTH, MOON, SUN
        return cls(almanac.frame_info(SUN), [almanac.frame_info(EARTH), almanac.frame_info(MOON)])

    def index_of(self, body) -> int:
        """Position in `shadow_bodies` of a Frame of the model (by NAIF id), or the index itself."""
        if isinstance(body, (int, np.integer)) and not isinstance(body, bool):
            if not 0 <= int(body) < len(self.shadow_bodies):
                raise ValueError(f"body index {int(body)} outside 0 .. {len(self.shadow_bodies) - 1}")
            return int(body)
        ids = [int(b.naif_id) for b in self.shadow_bodies]
        if int(body.naif_id) not in ids:
            raise ValueError(f"frame {int(body.naif_id)} is not a shadow body of this model")
        return ids.index(int(body.naif_id))


def check_shadow_model(model: ShadowModel, almanac, central) -> None:
    """What `check_ecl_series` (csrc/series_host.h) refuses, on the host: ValueError."""
    if not isinstance(model, ShadowModel):
        raise TypeError(f"{model!r} is not a ShadowModel")
    if not 1 <= len(model.shadow_bodies) <= MAX_BODIES:
        raise ValueError(f"shadow model: {len(model.shadow_bodies)} shadow bodies, 1 .. {MAX_BODIES} per call")
    for which, frame, least in [("light source", model.light_source, 1)] + [(f"shadow_bodies[{k}]", b, 0) for k, b in enumerate(model.shadow_bodies)]:
        checked_chain(body_chain(frame.naif_id, almanac, central), almanac, f"shadow model: the {which}", least,
                      " (the light source cannot be the central body)" if least else "")
        radius = float(frame.mean_equatorial_radius_km)
        if not (math.isfinite(radius) and radius > 0.0):
            raise ValueError(f"shadow model: the {which} needs a finite mean radius > 0")


def _asin_c(x: float) -> float:
    return math.asin(x) if -1.0 <= x <= 1.0 else math.nan   # (C's asin / acos: NaN out of range, no exception)


def _acos_c(x: float) -> float:
    return math.acos(x) if -1.0 <= x <= 1.0 else math.nan


_asin, _acos = _libm(_asin_c), _libm(_acos_c)


def body_position(naif_id: int, epoch_ns, almanac, central) -> np.ndarray:
    """`body_position` of the oracle: the signed sum over the chain, in chain order, from zero."""
    return chain_state(body_chain(naif_id, almanac, central), _ns_to_seconds(epoch_ns), almanac, with_v=False)[0]


def _norm3(v):
    return np.sqrt(v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2])


def _apparent(radius_km: float, dist):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(radius_km >= dist, radius_km, _asin(radius_km / dist))


def _circ_seg_area(r, d):
    return r * r * _acos(d / r) - d * np.sqrt(r * r - d * d)


def disk(r_back_km: float, r_front_km: float, r_eb, r_ls):
    """(pct, ls_p, fo_p, d_p) of `occultation_pct` (oracle/nyx_oracle.c:266-298), vectorised over the leading dimensions."""
    r_eb, r_ls = np.asarray(r_eb, dtype=np.float64), np.asarray(r_ls, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        n_ls, n_eb = _norm3(r_ls), _norm3(r_eb)
        ls_p, fo_p = _apparent(float(r_back_km), n_ls), _apparent(float(r_front_km), n_eb)
        dot = r_ls[..., 0] * r_eb[..., 0] + r_ls[..., 1] * r_eb[..., 1] + r_ls[..., 2] * r_eb[..., 2]
        d_p = _acos(-dot / (n_eb * n_ls))
        lit = d_p - ls_p > fo_p
        umbra = ~lit & (fo_p > d_p + ls_p)
        pen = ~lit & ~umbra & (np.abs(ls_p - fo_p) < d_p) & (d_p < ls_p + fo_p)
        d1 = (d_p * d_p - ls_p * ls_p + fo_p * fo_p) / (2.0 * d_p)
        d2 = (d_p * d_p + ls_p * ls_p - fo_p * fo_p) / (2.0 * d_p)
        # (the lens only where the formula takes it: elsewhere its acos arguments leave [-1, 1])
        shadow = np.full(d_p.shape, np.nan)
        if pen.any():
            shadow[pen] = _circ_seg_area(fo_p[pen], d1[pen]) + _circ_seg_area(ls_p[pen], d2[pen])
        nominal = 3.14159265358979323846 * (ls_p * ls_p)
        lens = np.where(np.isnan(shadow), 100.0, 100.0 * shadow / nominal)
        annular = 100.0 * (fo_p * fo_p) / (ls_p * ls_p)
        pct = np.where(lit, 0.0, np.where(umbra, 100.0, np.where(pen, lens, annular)))
    return pct, ls_p, fo_p, d_p


def eclipse_value(param, r, epoch_ns, model: ShadowModel, almanac, central, body=None) -> np.ndarray:
    """Value of `param` (EclipseParameter) for every row of `r` ([..., 3] or [..., 6], km, in the frame of `central`) at
    `epoch_ns` (broadcast).  `body` (a Frame of the model or its index) names the body of a per-body parameter.  The
    definition the device kernel is tested against."""
    param = EclipseParameter(param)
    check_shadow_model(model, almanac, central)
    r = np.asarray(r, dtype=np.float64)[..., :3]
    epoch = np.broadcast_to(np.asarray(epoch_ns, dtype=np.int64), r.shape[:-1])
    ps = body_position(model.light_source.naif_id, epoch, almanac, central)
    r_ls = ps - r
    r_sun = float(model.light_source.mean_equatorial_radius_km)
    if param is EclipseParameter.SunRange:
        return _norm3(r_ls)
    if param is EclipseParameter.SunApparentRadius:
        return _apparent(r_sun, _norm3(r_ls)) * _TO_DEG

    def one(b):
        frame = model.shadow_bodies[b]
        return disk(r_sun, float(frame.mean_equatorial_radius_km), r - body_position(frame.naif_id, epoch, almanac, central), r_ls)

    if param in PER_BODY:
        if body is None:
            raise ValueError(f"{param.name} is a per-body parameter: name the body")
        pct, ls_p, fo_p, d_p = one(model.index_of(body))
        if param is EclipseParameter.BodyOccultation:
            return pct
        if param is EclipseParameter.BodyApparentRadius:
            return fo_p * _TO_DEG
        if param is EclipseParameter.BodySeparation:
            return d_p * _TO_DEG
        if param is EclipseParameter.BodyPenumbraMargin:
            return ((d_p - ls_p) - fo_p) * _TO_DEG
        return (fo_p - (d_p + ls_p)) * _TO_DEG
    best, winner = np.zeros(r.shape[:-1]), np.full(r.shape[:-1], -1.0)
    nan = np.zeros(r.shape[:-1], dtype=bool)
    for b in range(len(model.shadow_bodies)):
        pct = one(b)[0]
        nan |= np.isnan(pct)
        with np.errstate(invalid="ignore"):
            more = pct > best
        best, winner = np.where(more, pct, best), np.where(more, float(b), winner)
    nan |= np.isnan(r_ls).any(axis=-1)
    if param is EclipseParameter.Occultation:
        out = best
    elif param is EclipseParameter.Illumination:
        out = np.abs(best / 100.0 - 1.0)
    elif param is EclipseParameter.State:
        out = np.where(best == 0.0, 0.0, np.where(best == 100.0, 2.0, 1.0))
    else:
        out = winner
    return np.where(nan, np.nan, out)


def state_changes(occultation, length=None) -> np.ndarray:
    """Per run (column of occultation[K, runs]), the number of samples k >= 1, k < length, whose Occultation differs from the
    previous sample's: the count the reference's tests assert along a propagated trajectory (tests/cosmic/eclipse.rs)."""
    occ = np.asarray(occultation, dtype=np.float64)
    if occ.ndim == 1:
        occ = occ[:, None]
    k, runs = occ.shape
    length = np.full(runs, k, dtype=np.int64) if length is None else np.minimum(np.asarray(length, dtype=np.int64), k)
    if k < 2:
        return np.zeros(runs, dtype=np.int64)
    held = np.arange(1, k)[:, None] < length[None, :]
    return ((occ[1:] != occ[:-1]) & held).sum(axis=0).astype(np.int64)
