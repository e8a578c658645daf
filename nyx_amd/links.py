"""Links: the range, the Doppler and the line of sight from one spacecraft to another, and which body blocks it.

Host-side definition of what `InterlinkTxSpacecraft::measure_instantaneous` (od/interlink/trk_device.rs) forms for a receiver
seen from a transmitter, both given in the inertial frame of one centre.  The device kernel (csrc/link_kernel.hip, csrc/link_dev.h)
is tested against this module, which states every value OPERATION FOR OPERATION in float64 - sums of three as ((a0 + a1) + a2),
one rounding per operation, only + - * / sqrt and comparisons - so that the two agree bit for bit.

    rho = r_rx - r_tx
    Range |rho|;  RangeRate rho . (v_rx - v_tx) / |rho|;  RelativeSpeed |v_rx - v_tx|;  Los rho / |rho| (transmitter to receiver)
    ReferenceDoppler rho . v_rx / |rho|: what the reference forms AS WRITTEN - it transforms the receiver into
        `observer.orbit.frame`, the common centre and not the transmitter, so the velocity is the receiver's own

Obstruction is Vallado's SIGHT test, which the reference's `almanac.line_of_sight_obstructed` call implements; anise's source is not
part of the reference tree, so this restates the published formula and is not pinned against anise.  With b the body's position
(the signed sum of the almanac's Chebyshev segments along its chain, in chain order; zero for the centre), r1 = r_rx - b,
r2 = r_tx - b and R its mean radius:

    tau = (r1.r1 - r1.r2) / ((r1.r1 + r2.r2) - 2 r1.r2)
    d2  = tau < 0 ? r1.r1 : (tau > 1 ? r2.r2 : (1 - tau) r1.r1 + r1.r2 tau)
    obstructs = 0 <= tau <= 1 and d2 <= R R;   BodyClearance = sqrt(d2) - R

Coincident spacecraft give a NaN tau: not obstructed, BodyClearance NaN, RangeRate NaN.  Not guarded.  An epoch outside a segment
of a chain in use gives NaN for that sample (the device series ends there).  Out of scope: light time, aberration, noise, the
integration-time average of `measure`, antenna masks.
"""
from __future__ import annotations

import enum
import math

import numpy as np

from .chains import MAX_CHAIN, body_chain, checked_chain  # noqa: F401  (re-exported)
from .eclipse import body_position


class LinkParameter(enum.IntEnum):
    """enum nyx_hip_link_param (include/nyx_hip_link.h): never renumber."""

    Range = 0               # km
    RangeRate = 1           # km/s, the physical one
    ReferenceDoppler = 2    # km/s, the reference's value as written
    Visible = 3             # 1.0 when no body obstructs, else 0.0
    ObstructingBody = 4     # index of the first body that obstructs, else -1.0
    Clearance = 5           # km: the minimum over the bodies of BodyClearance (+inf without bodies; a NaN never wins)
    RelativeSpeed = 6       # km/s
    LosX = 7                # rho / |rho|, transmitter to receiver, inertial
    LosY = 8
    LosZ = 9
    # of ONE body
    BodyClearance = 10      # km: sqrt(d2) - R
    BodyObstructs = 11      # 1.0 / 0.0


PER_BODY = frozenset((LinkParameter.BodyClearance, LinkParameter.BodyObstructs))
DEFAULT_PARAMS = (LinkParameter.Range, LinkParameter.RangeRate, LinkParameter.Visible)
MAX_BODIES = 8


def default_bodies(central) -> list:
    """What the reference obstructs with: the transmitter's orbit frame - the centre with its mean equatorial radius."""
    return [central]


def body_index(bodies, body) -> int:
    """Position in `bodies` of a Frame (by NAIF id), or the index itself."""
    if isinstance(body, (int, np.integer)) and not isinstance(body, bool):
        if not 0 <= int(body) < len(bodies):
            raise ValueError(f"body index {int(body)} outside 0 .. {len(bodies) - 1}")
        return int(body)
    ids = [int(b.naif_id) for b in bodies]
    if int(body.naif_id) not in ids:
        raise ValueError(f"frame {int(body.naif_id)} is not one of the bodies of this link")
    return ids.index(int(body.naif_id))


def link_chain(frame, almanac, central):
    """[(segment, sign), ...] of a body of a link; [] for the centre, which needs no almanac."""
    if int(frame.naif_id) == int(central.naif_id):
        return []
    if almanac is None:
        raise ValueError(f"body {int(frame.naif_id)} is not the centre: its position needs an almanac")
    return body_chain(frame.naif_id, almanac, central)


def check_link_bodies(bodies, almanac, central) -> None:
    """What `check_link_series` (csrc/series_host.h) refuses of the bodies, on the host: ValueError.  An almanac is needed only when
    a body has a chain (is not the centre)."""
    bodies = list(bodies)
    if len(bodies) > MAX_BODIES:
        raise ValueError(f"link: {len(bodies)} bodies, 0 .. {MAX_BODIES} per call")
    for k, frame in enumerate(bodies):
        checked_chain(link_chain(frame, almanac, central), almanac, f"link: bodies[{k}]")
        radius = float(frame.mean_equatorial_radius_km)
        if not (math.isfinite(radius) and radius > 0.0):
            raise ValueError(f"link: bodies[{k}] needs a finite mean radius > 0")


def link_param(param, bodies=None):
    """(LinkParameter, body index) of a LinkParameter, or of a pair (per-body LinkParameter, frame or index)."""
    body = None
    if isinstance(param, tuple):
        param, body = param
    if not isinstance(param, LinkParameter):
        raise TypeError(f"{param!r} is not a LinkParameter")
    if param in PER_BODY:
        if body is None or bodies is None:
            raise ValueError(f"{param.name} is a per-body parameter: give it as ({param.name}, frame_or_index)")
        if not len(bodies):
            raise ValueError(f"{param.name} is a per-body parameter and the link names no body")
        return param, body_index(bodies, body)
    if body is not None:
        raise ValueError(f"{param.name} is a parameter of the whole link: it takes no body")
    return param, 0


def _dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def sight(r_rx, r_tx, b, radius_km: float):
    """(tau, d2, obstructs, clearance) of one body at `b`, vectorised over the leading dimensions."""
    r1, r2 = r_rx - b, r_tx - b
    with np.errstate(invalid="ignore", divide="ignore"):
        r1sq, r2sq, d = _dot3(r1, r1), _dot3(r2, r2), _dot3(r1, r2)
        tau = (r1sq - d) / ((r1sq + r2sq) - 2.0 * d)
        d2 = np.where(tau < 0.0, r1sq, np.where(tau > 1.0, r2sq, (1.0 - tau) * r1sq + d * tau))
        obstructs = (tau >= 0.0) & (tau <= 1.0) & (d2 <= float(radius_km) * float(radius_km))
        clearance = np.sqrt(d2) - float(radius_km)
    return tau, d2, obstructs, clearance


def outside_ephemerides(epoch_ns, bodies, almanac, central) -> np.ndarray:
    """True where an epoch lies outside a segment of the chain of one of `bodies` (None: the centre, which has none): the sample
    at which a device series ends."""
    epoch = np.asarray(epoch_ns, dtype=np.int64)
    out = np.zeros(epoch.shape, dtype=bool)
    for frame in (default_bodies(central) if bodies is None else bodies):
        if link_chain(frame, almanac, central):
            out |= np.isnan(body_position(frame.naif_id, epoch, almanac, central)).any(axis=-1)
    return out


def link_value(param, rv_rx, rv_tx, epoch_ns, bodies, almanac, central, body=None) -> np.ndarray:
    """Value of `param` (LinkParameter) for every row of `rv_rx` / `rv_tx` ([..., 6], km and km/s, receiver and transmitter in the
    frame of `central`; broadcast against each other) at `epoch_ns` (broadcast).  `bodies`: the Frames that can block the line
    (None: the centre); `body` (one of them, or its index) names the body of a per-body parameter.  The definition the device
    kernel is tested against."""
    param = LinkParameter(param)
    bodies = default_bodies(central) if bodies is None else list(bodies)
    check_link_bodies(bodies, almanac, central)
    rx, tx = np.broadcast_arrays(np.asarray(rv_rx, dtype=np.float64), np.asarray(rv_tx, dtype=np.float64))
    shape = rx.shape[:-1]
    rho = rx[..., :3] - tx[..., :3]
    with np.errstate(invalid="ignore", divide="ignore"):
        if param is LinkParameter.Range:
            return np.sqrt(_dot3(rho, rho))
        if param is LinkParameter.RangeRate:
            return _dot3(rho, rx[..., 3:] - tx[..., 3:]) / np.sqrt(_dot3(rho, rho))
        if param is LinkParameter.ReferenceDoppler:
            return _dot3(rho, rx[..., 3:]) / np.sqrt(_dot3(rho, rho))
        if param is LinkParameter.RelativeSpeed:
            dv = rx[..., 3:] - tx[..., 3:]
            return np.sqrt(_dot3(dv, dv))
        if param in (LinkParameter.LosX, LinkParameter.LosY, LinkParameter.LosZ):
            return rho[..., int(param) - int(LinkParameter.LosX)] / np.sqrt(_dot3(rho, rho))
    epoch = np.broadcast_to(np.asarray(epoch_ns, dtype=np.int64), shape)

    def one(b):
        frame = bodies[b]
        pos = body_position(frame.naif_id, epoch, almanac, central) if link_chain(frame, almanac, central) else np.zeros(shape + (3,))
        return sight(rx[..., :3], tx[..., :3], pos, float(frame.mean_equatorial_radius_km)), np.isnan(pos).any(axis=-1)

    if param in PER_BODY:
        if body is None:
            raise ValueError(f"{param.name} is a per-body parameter: name the body")
        (_, _, obstructs, clearance), outside = one(body_index(bodies, body))
        return np.where(outside, np.nan, clearance if param is LinkParameter.BodyClearance else np.where(obstructs, 1.0, 0.0))
    first, best = np.full(shape, -1.0), np.full(shape, np.inf)
    nan = np.zeros(shape, dtype=bool)
    for b in range(len(bodies)):
        (_, _, obstructs, clearance), outside = one(b)
        nan |= outside
        first = np.where(obstructs & (first < 0.0), float(b), first)
        with np.errstate(invalid="ignore"):
            best = np.where(clearance < best, clearance, best)
    if param is LinkParameter.Visible:
        out = np.where(first < 0.0, 1.0, 0.0)
    elif param is LinkParameter.ObstructingBody:
        out = first
    else:
        out = best
    return np.where(nan, np.nan, out)
