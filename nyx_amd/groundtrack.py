"""Ground tracks: the state expressed in a body-fixed frame, as geodetic latitude / longitude / height.

Host-side definition of what `Traj::to_groundtrack_parquet` (md/trajectory/sc_traj.rs:131-155) writes - the trajectory
in the body-fixed frame, one state per step, as geodetic latitude, longitude, height and |r| - and of the other values a
body-fixed state gives (declination, its Cartesian components, the ground-relative speed).  The device kernel
(csrc/groundtrack_kernel.hip) reuses the code of the stop conditions (csrc/event_dev.h: `ev_to_frame`, `ev_geodetic`,
`ev_scalar`); this module restates those OPERATION FOR OPERATION and is what the kernel is tested against:

* sums of three are taken left to right, a0 + a1 + a2, as in `ev_to_frame` / `ev_scalar` (not in `state_value`'s
  numpy-axis order);
* sin / cos / atan2 / asin are the C library's (`math`), element by element, not numpy's vector loops: the same functions
  the oracle calls, whatever SIMD paths a numpy build selects.

A ground-track `Height` therefore equals the `Height` event scalar of the same state and frame: a run stopped with
`until_event(Height = h)` reports h at its last sample, within the event's own precision.

ONE DELIBERATE DIFFERENCE FROM THE REFERENCE.  The reference rotates the STORED states (`to_frame`) and then interpolates
in the rotating frame.  Here the inertial state is interpolated (`traj_at`, bit-identical to `traj_every`) and rotated AT
THE SAMPLE EPOCH: no interpolation error is added by the frame's rotation, and the two orders differ by interpolation
error only.  That error is NOT always small: 2e-7 km where the stored steps are even, but kilometres (134.8 km at worst on
one LEO orbit) in windows that hold states a few seconds apart - the step controller at a shadow crossing - and in the
last interval, where the 13-state interpolant itself is kilometres from the propagated state in either frame; the inertial
order is the closer of the two there (measured in tests/test_groundtrack_host.py, DESIGN.md "Ground tracks").

Frames: `Rotation`s of the IAU kind (phase-angle polynomials with their nutation-precession series) of the SAME centre
as the states.  A `Rotation` with `euler` set, or a frame of another centre, raises NotImplementedError;
`frame.rotation is None` is the identity orientation - the values are taken on the inertial state.
"""
from __future__ import annotations

import enum
import math

import numpy as np


class GroundTrackParameter(enum.Enum):
    """What a ground track can hold; every member is evaluated on the state expressed in the body-fixed frame."""

    Latitude = "Latitude"        # geodetic, deg
    Longitude = "Longitude"      # deg, [0, 360)
    Height = "Height"            # geodetic, km
    Rmag = "Rmag"                # km
    Declination = "Declination"  # deg: asin(z / |r|)
    X = "X"                      # km
    Y = "Y"
    Z = "Z"
    VX = "VX"                    # km/s, relative to the rotating frame
    VY = "VY"
    VZ = "VZ"
    Vmag = "Vmag"                # km/s: the ground-relative speed


GEODETIC = (GroundTrackParameter.Latitude, GroundTrackParameter.Height)
# the reference's four fields (sc_traj.rs:131-155)
DEFAULT_PARAMS = (GroundTrackParameter.Latitude, GroundTrackParameter.Longitude, GroundTrackParameter.Height, GroundTrackParameter.Rmag)

_CART = {GroundTrackParameter.X: 0, GroundTrackParameter.Y: 1, GroundTrackParameter.Z: 2, GroundTrackParameter.VX: 3,
         GroundTrackParameter.VY: 4, GroundTrackParameter.VZ: 5}

_DEG = 3.14159265358979323846 / 180.0
_HALF_PI = 1.57079632679489661923
_TO_DEG = 180.0 / 3.14159265358979323846
_NS_PER_CENTURY = 3155760000 * 10**9


def _libm(fn, nin=1):
    u = np.frompyfunc(fn, nin, 1)
    return lambda *a: np.asarray(u(*a), dtype=np.float64)


_sin, _cos, _asin, _atan2 = _libm(math.sin), _libm(math.cos), _libm(math.asin), _libm(math.atan2, 2)


def _ns_to_seconds(epoch_ns) -> np.ndarray:
    """`ns_to_seconds` of csrc/hifitime_dev.h (`Duration::to_seconds`): centuries, whole seconds and the sub-second part."""
    ns = np.asarray(epoch_ns, dtype=np.int64)
    cent = np.floor_divide(ns, _NS_PER_CENTURY)
    rem = ns - cent * _NS_PER_CENTURY
    whole, sub = np.floor_divide(rem, 10**9), np.mod(rem, 10**9)
    near = whole.astype(np.float64) + sub.astype(np.float64) * 1e-9
    return np.where(cent == 0, near, cent.astype(np.float64) * 3155760000.0 + whole.astype(np.float64) + sub.astype(np.float64) * 1e-9)


def check_frame(frame, central_naif_id=None, params=()):
    """The refusals of the device path, on the host: Euler-Chebyshev orientations and frames of another centre raise
    NotImplementedError (the wording `Event` uses), a geodetic parameter without an ellipsoid raises ValueError."""
    rot = getattr(frame, "rotation", None)
    if rot is not None and rot.euler is not None:
        raise NotImplementedError("ground-track frames are IAU-oriented frames on the device path")
    if central_naif_id is not None and int(frame.naif_id) != int(central_naif_id):
        raise NotImplementedError(f"ground-track frames are IAU-oriented frames of the same centre on the device path "
                                  f"(frame {frame.naif_id}, trajectories around {central_naif_id})")
    if any(p in GEODETIC for p in params):
        if not float(frame.mean_equatorial_radius_km) > 0.0:
            raise ValueError("Latitude / Height need the frame's equatorial radius (mean_equatorial_radius_km > 0)")
    if not 0.0 <= float(frame.flattening) < 1.0:
        raise ValueError("the frame's flattening must be in [0, 1)")


def iau_dcm(rotation, epoch_ns):
    """(dcm[..., 3, 3], wdot_rad_s[...]) of an IAU orientation at `epoch_ns` (any shape): `ev_to_frame` of csrc/event_dev.h
    restated - the same et / d / T, the same order of the polynomial sums, the same nutation-precession loop, and
    DCM = R3(W) R1(90 - delta) R3(90 + alpha), integration frame -> body-fixed.  `rotation=None`: the identity, rate 0."""
    et = _ns_to_seconds(epoch_ns)
    if rotation is None:
        return np.broadcast_to(np.eye(3), et.shape + (3, 3)).copy(), np.zeros(et.shape)
    if rotation.euler is not None:
        raise NotImplementedError("ground-track frames are IAU-oriented frames on the device path")
    ra_c, dec_c, w_c = ([float(x) for x in c] for c in (rotation.ra_deg, rotation.dec_deg, rotation.w_deg))
    d, T = et / 86400.0, et / (86400.0 * 36525.0)
    ra = ra_c[0] + ra_c[1] * T + ra_c[2] * T * T
    dec = dec_c[0] + dec_c[1] * T + dec_c[2] * T * T
    w = w_c[0] + w_c[1] * d + w_c[2] * d * d
    wd = w_c[1] + 2.0 * w_c[2] * d
    n = len(rotation.nut_prec_angles_deg)
    coef = lambda seq, k: float(seq[k]) if k < len(seq) else 0.0
    for k in range(n):
        a0, a1 = float(rotation.nut_prec_angles_deg[k][0]), float(rotation.nut_prec_angles_deg[k][1])
        th = (a0 + a1 * T) * _DEG
        sn, cs = _sin(th), _cos(th)
        ra = ra + coef(rotation.nut_prec_ra, k) * sn
        dec = dec + coef(rotation.nut_prec_dec, k) * cs
        w = w + coef(rotation.nut_prec_w, k) * sn
        wd = wd + coef(rotation.nut_prec_w, k) * cs * (a1 * _DEG / 36525.0)
    a1_, a2_, a3_ = _HALF_PI + ra * _DEG, _HALF_PI - dec * _DEG, w * _DEG
    s1, c1, s2, c2, s3, c3 = _sin(a1_), _cos(a1_), _sin(a2_), _cos(a2_), _sin(a3_), _cos(a3_)
    m = np.stack([c3 * c1 - s3 * c2 * s1, c3 * s1 + s3 * c2 * c1, s3 * s2,
                  -s3 * c1 - c3 * c2 * s1, -s3 * s1 + c3 * c2 * c1, c3 * s2,
                  s2 * s1, -s2 * c1, c2], axis=-1)
    return m.reshape(et.shape + (3, 3)), wd * _DEG / 86400.0


def to_body_fixed(rv, epoch_ns, frame) -> np.ndarray:
    """`rv` ([..., 6], km and km/s, in the integration frame) expressed in the body-fixed `frame` at `epoch_ns` (broadcast
    against the leading dimensions): position R r, velocity R v - w x (R r) with w = dW/dt about the frame's pole.  Like
    the event path (`ev_to_frame`) this NEGLECTS THE DRIFT OF THE POLE itself (d alpha / dt, d delta / dt: about 2e-8 km/s
    at the Earth's surface).  `frame.rotation is None`: a copy of `rv`."""
    rv = np.asarray(rv, dtype=np.float64)
    rot = getattr(frame, "rotation", None)
    if rot is None:
        return rv.copy()
    epoch = np.broadcast_to(np.asarray(epoch_ns, dtype=np.int64), rv.shape[:-1])
    m, wdot = iau_dcm(rot, epoch)
    out = np.empty(rv.shape, dtype=np.float64)
    for i in range(3):
        out[..., i] = m[..., i, 0] * rv[..., 0] + m[..., i, 1] * rv[..., 1] + m[..., i, 2] * rv[..., 2]
        out[..., 3 + i] = m[..., i, 0] * rv[..., 3] + m[..., i, 1] * rv[..., 4] + m[..., i, 2] * rv[..., 5]
    out[..., 3] = out[..., 3] + wdot * out[..., 1]
    out[..., 4] = out[..., 4] - wdot * out[..., 0]
    return out


def geodetic(r_fixed, eq_radius_km: float, flattening: float):
    """(lat_deg[...], height_km[...]) of body-fixed positions ([..., 3] or [..., 6]) on the ellipsoid (a, f): `ev_geodetic`
    restated - the classical iteration (Vallado, Algorithm 12) from the geocentric latitude, at most 20 passes, stopped
    once a pass moves the latitude by less than 1e-12 rad; the height from r_delta / cos(lat), or near the poles
    (|cos(lat)| <= 1e-6) from |z| / |sin(lat)|."""
    y = np.asarray(r_fixed, dtype=np.float64)
    a, f = float(eq_radius_km), float(flattening)
    e2 = f * (2.0 - f)
    r_delta = np.sqrt(y[..., 0] * y[..., 0] + y[..., 1] * y[..., 1])
    z = y[..., 2]
    lat = _atan2(z, r_delta)
    active = np.ones(lat.shape, dtype=bool)
    with np.errstate(invalid="ignore", divide="ignore"):
        for _ in range(20):
            sl = _sin(lat)
            c = a / np.sqrt(1.0 - e2 * sl * sl)
            nl = _atan2(z + c * e2 * sl, r_delta)
            done = np.abs(nl - lat) < 1e-12
            lat = np.where(active, nl, lat)      # (an element that has stopped keeps its latitude: its lane left the loop)
            active = active & ~done
            if not active.any():
                break
        lat_deg = lat * _TO_DEG
        sl, cl = _sin(lat), _cos(lat)
        c = a / np.sqrt(1.0 - e2 * sl * sl)
        height = np.where(np.abs(cl) > 1e-6, r_delta / cl - c, np.abs(z) / np.abs(sl) - c * (1.0 - e2))
    return lat_deg, height


def longitude_deg(r_fixed) -> np.ndarray:
    """atan2(y, x) in degrees in [0, 360), as the Longitude event scalar; y = -0.0 gives 0.  A negative angle smaller than
    half an ulp of 360, which `deg + 360` would round to 360 itself, is 0."""
    y = np.asarray(r_fixed, dtype=np.float64)
    deg = _atan2(y[..., 1], y[..., 0]) * _TO_DEG
    w = np.where(deg < 0.0, deg + 360.0, deg)
    return np.where(w >= 360.0, 0.0, w)


def body_fixed_value(param: GroundTrackParameter, yf, eq_radius_km: float = 0.0, flattening: float = 0.0) -> np.ndarray:
    """`param` of states ALREADY expressed in the body-fixed frame ([..., 6])."""
    yf = np.asarray(yf, dtype=np.float64)
    if not isinstance(param, GroundTrackParameter):
        raise TypeError(f"{param!r} is not a GroundTrackParameter")
    if param in _CART:
        return yf[..., _CART[param]].copy()
    if param is GroundTrackParameter.Longitude:
        return longitude_deg(yf)
    if param in GEODETIC:
        if not float(eq_radius_km) > 0.0:
            raise ValueError("Latitude / Height need the frame's equatorial radius (mean_equatorial_radius_km > 0)")
        lat, h = geodetic(yf, eq_radius_km, flattening)
        return lat if param is GroundTrackParameter.Latitude else h
    if param is GroundTrackParameter.Vmag:
        return np.sqrt(yf[..., 3] * yf[..., 3] + yf[..., 4] * yf[..., 4] + yf[..., 5] * yf[..., 5])
    rmag = np.sqrt(yf[..., 0] * yf[..., 0] + yf[..., 1] * yf[..., 1] + yf[..., 2] * yf[..., 2])
    if param is GroundTrackParameter.Rmag:
        return rmag
    with np.errstate(invalid="ignore", divide="ignore"):
        return _asin(yf[..., 2] / rmag) * _TO_DEG      # Declination


def ground_track_value(param: GroundTrackParameter, rv, epoch_ns, frame) -> np.ndarray:
    """Value of `param` for every row of `rv` ([..., 6], integration frame) at `epoch_ns` (broadcast) in `frame`:
    `to_body_fixed`, then the event scalar of that name.  The definition the device kernel is tested against."""
    check_frame(frame, params=(param,))
    return body_fixed_value(param, to_body_fixed(rv, epoch_ns, frame), frame.mean_equatorial_radius_km, frame.flattening)
