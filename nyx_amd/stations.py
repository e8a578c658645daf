"""Station views: azimuth, elevation, range and range rate of a state seen from a ground station.

Host-side definition of what `GroundStation::azimuth_elevation_of` / `TrackingDevice::measure_instantaneous`
(od/ground_station/mod.rs:69-105, od/ground_station/trk_device.rs:158-208) compute - the station placed by geodetic latitude /
longitude / height in an IAU body-fixed frame, the spacecraft expressed in that frame, azimuth / elevation / range / range rate
in the station's south-east-zenith (SEZ) triad, the measurement kept when the elevation is above the station's mask.  The
device kernel (csrc/aer_kernel.hip) is tested against this module, which restates it OPERATION FOR OPERATION:

* the station constants (`station_consts`: body-fixed position, triad, mask) are what `aer_station_consts` of csrc/aer_args.h
  computes on the host with the C library - the same operations in the same order, products left to right, so the two agree
  bit for bit;
* per sample, sums of three are taken left to right, a0 + a1 + a2, and asin / atan2 are the C library's (`math`), element by
  element, as in `groundtrack.py`.

A RESTATEMENT, NOT A PINNED PARITY.  The reference delegates the geometry to anise (`azimuth_elevation_range_sez`,
`Orbit::try_latlongalt`), which is not part of the reference tree: the formulas here are the published ones (Vallado, section
4.4.3 and Algorithm 27) and are not checked against anise's output.

    C = a / sqrt(1 - e^2 sin^2 phi),  S = C (1 - e^2),  e^2 = f (2 - f)
    r_st = [(C + h) cos phi cos lambda, (C + h) cos phi sin lambda, (S + h) sin phi]
    S^ = [sin phi cos lambda, sin phi sin lambda, -cos phi],  E^ = [-sin lambda, cos lambda, 0],
    Z^ = [cos phi cos lambda, cos phi sin lambda, sin phi]
    rho = r_fixed - r_st;  range = |(rho.S^, rho.E^, rho.Z^)|;  elevation = asin(rho.Z^ / range)
    azimuth = atan2(rho.E^, -rho.S^) in [0, 360);  range_rate = rho . v_fixed / range   (the station is at rest in the frame)

The frame is the one of the ground tracks (`groundtrack.to_body_fixed`): the drift of the pole itself is neglected, which enters
the range rate with at most 5e-8 km/s at the Earth's surface - three orders below the reference's Doppler noise (5e-5 km/s).
No light-time correction, no terrain mask beyond one constant elevation, no obstruction by another body.
"""
from __future__ import annotations

import enum
import math
from dataclasses import dataclass

import numpy as np

from .groundtrack import _DEG, _TO_DEG, _atan2, _libm, check_frame, to_body_fixed


class AerParameter(enum.Enum):
    """What a station view can hold."""

    Azimuth = "Azimuth"                        # deg, [0, 360), from north through east
    Elevation = "Elevation"                    # deg
    Range = "Range"                            # km
    RangeRate = "RangeRate"                    # km/s
    ElevationAboveMask = "ElevationAboveMask"  # deg: elevation - the station's mask
    Visible = "Visible"                        # 1.0 where elevation >= mask, else 0.0 (a NaN elevation is not visible)
    RhoS = "RhoS"                              # km: the line of sight in the station's SEZ triad
    RhoE = "RhoE"
    RhoZ = "RhoZ"


# what `MeasurementType::compute_one_way` reads (od/msr/types.rs:102-117)
DEFAULT_PARAMS = (AerParameter.Azimuth, AerParameter.Elevation, AerParameter.Range, AerParameter.RangeRate)


@dataclass
class GroundStation:
    """A station on the ellipsoid of the body-fixed `frame` (od/ground_station/mod.rs:39-66, the geometry only)."""

    name: str
    latitude_deg: float          # geodetic, [-90, 90]
    longitude_deg: float
    height_km: float             # above the ellipsoid
    frame: object                # an IAU-oriented Frame of the trajectories' centre, with its ellipsoid
    elevation_mask_deg: float = 0.0


@dataclass
class StationConsts:
    """What the kernel reads of one station, in body-fixed components (`AerStationConsts` of csrc/aer_args.h)."""

    r_km: tuple
    south: tuple
    east: tuple
    zenith: tuple
    mask_deg: float


def _asin_c(x: float) -> float:
    return math.asin(x) if -1.0 <= x <= 1.0 else math.nan   # (C's asin: NaN for a NaN or out-of-range argument, no exception)


_asin = _libm(_asin_c)


def station_consts(station: GroundStation) -> StationConsts:
    """`aer_station_consts` of csrc/aer_args.h restated: the same operations in the same order, with the C library's sin / cos."""
    a, f = float(station.frame.mean_equatorial_radius_km), float(station.frame.flattening)
    h = float(station.height_km)
    e2 = f * (2.0 - f)
    phi, lam = float(station.latitude_deg) * _DEG, float(station.longitude_deg) * _DEG
    sp, cp, sl, cl = math.sin(phi), math.cos(phi), math.sin(lam), math.cos(lam)
    c = a / math.sqrt(1.0 - e2 * sp * sp)
    sz = c * (1.0 - e2)
    return StationConsts(r_km=((c + h) * cp * cl, (c + h) * cp * sl, (sz + h) * sp), south=(sp * cl, sp * sl, -cp), east=(-sl, cl, 0.0),
                         zenith=(cp * cl, cp * sl, sp), mask_deg=float(station.elevation_mask_deg))


def check_station(station: GroundStation, index: int = 0) -> None:
    """The refusals of `check_aer_series` (csrc/series_host.h) for one station, on the host."""
    if not isinstance(station, GroundStation):
        raise TypeError(f"stations[{index}] = {station!r} is not a GroundStation")
    if not -90.0 <= float(station.latitude_deg) <= 90.0:
        raise ValueError(f"stations[{index}] ({station.name}): latitude_deg must be in [-90, 90]")
    if not math.isfinite(float(station.longitude_deg)) or not math.isfinite(float(station.height_km)):
        raise ValueError(f"stations[{index}] ({station.name}): longitude_deg and height_km must be finite")
    if not -90.0 <= float(station.elevation_mask_deg) <= 90.0:
        raise ValueError(f"stations[{index}] ({station.name}): elevation_mask_deg must be in [-90, 90]")


def check_stations(stations, central_naif_id=None):
    """The refusals of the device path, on the host -> the one frame all `stations` share.  No station, a station of another
    frame than the first, a latitude or a mask outside [-90, 90], a non-finite longitude or height and a frame without an
    ellipsoid raise ValueError; Euler-Chebyshev orientations and frames of another centre raise NotImplementedError
    (`groundtrack.check_frame`)."""
    stations = list(stations)
    if not stations:
        raise ValueError("station views: at least one station")
    for k, st in enumerate(stations):
        check_station(st, k)
    frame = stations[0].frame
    for k, st in enumerate(stations):
        if st.frame is not frame and st.frame != frame:
            raise ValueError(f"stations[{k}] ({st.name}): all stations of one call share one frame")
    check_frame(frame, central_naif_id)
    if not float(frame.mean_equatorial_radius_km) > 0.0:
        raise ValueError("station views need the frame's equatorial radius (mean_equatorial_radius_km > 0): the stations stand on its ellipsoid")
    return frame


def sez_value(param: AerParameter, yf, consts: StationConsts) -> np.ndarray:
    """`param` of states ALREADY expressed in the station's body-fixed frame ([..., 6])."""
    if not isinstance(param, AerParameter):
        raise TypeError(f"{param!r} is not an AerParameter")
    yf = np.asarray(yf, dtype=np.float64)
    rx, ry, rz = yf[..., 0] - consts.r_km[0], yf[..., 1] - consts.r_km[1], yf[..., 2] - consts.r_km[2]
    dot = lambda u: rx * u[0] + ry * u[1] + rz * u[2]
    rho_s, rho_e, rho_z = dot(consts.south), dot(consts.east), dot(consts.zenith)
    if param is AerParameter.RhoS:
        return rho_s
    if param is AerParameter.RhoE:
        return rho_e
    if param is AerParameter.RhoZ:
        return rho_z
    rng = np.sqrt(rho_s * rho_s + rho_e * rho_e + rho_z * rho_z)
    if param is AerParameter.Range:
        return rng
    if param is AerParameter.Azimuth:   # the wrap of `groundtrack.longitude_deg`
        deg = _atan2(rho_e, -rho_s) * _TO_DEG
        w = np.where(deg < 0.0, deg + 360.0, deg)
        return np.where(w >= 360.0, 0.0, w)
    with np.errstate(invalid="ignore", divide="ignore"):
        if param is AerParameter.RangeRate:
            return (rx * yf[..., 3] + ry * yf[..., 4] + rz * yf[..., 5]) / rng
        el = _asin(rho_z / rng) * _TO_DEG
        if param is AerParameter.Elevation:
            return el
        above = el - consts.mask_deg
        if param is AerParameter.ElevationAboveMask:
            return above
        return np.where(above >= 0.0, 1.0, 0.0)      # Visible


def aer_value(param: AerParameter, rv, epoch_ns, station: GroundStation) -> np.ndarray:
    """Value of `param` for every row of `rv` ([..., 6], integration frame) at `epoch_ns` (broadcast) seen from `station`:
    `groundtrack.to_body_fixed` in the station's frame, then the SEZ geometry.  The definition the device kernel is tested
    against."""
    check_stations([station])
    return sez_value(param, to_body_fixed(rv, epoch_ns, station.frame), station_consts(station))
