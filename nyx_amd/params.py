"""`StateParameter` and `Spacecraft::value` for arrays of states.

Host-side mirror of what the Monte Carlo results hand to their consumers (`Results::every_value_of`,
`first_values_of`, ... nyx-core/src/mc/results.rs:86-245): the value of one state parameter for every resampled
state of every run.  `Spacecraft::value` (cosmic/spacecraft.rs:520-578) answers Cd / Cr / masses itself and
forwards `StateParameter::Element(e)` to ANISE's `OrbitalElement::evaluate` (the `analysis` feature, not part of
this reference tree): the Cartesian components and magnitudes are exact restatements; the Keplerian elements
follow ANISE's documented definitions (osculating elements from the Cartesian state and the frame's mu,
angles in degrees in [0, 360)) and are **parity unpinned** like the event scalars.
"""
from __future__ import annotations

import enum

import numpy as np


class StateParameter(enum.Enum):
    """md/param.rs:34-: the parameters this path can evaluate (Element(..) flattened to its element)."""

    X = "X"
    Y = "Y"
    Z = "Z"
    VX = "VX"
    VY = "VY"
    VZ = "VZ"
    Rmag = "Rmag"
    Vmag = "Vmag"
    Hmag = "Hmag"
    Energy = "Energy"
    SemiMajorAxis = "SemiMajorAxis"
    Eccentricity = "Eccentricity"
    Inclination = "Inclination"
    RAAN = "RAAN"
    AoP = "AoP"
    TrueAnomaly = "TrueAnomaly"
    Period = "Period"
    ApoapsisRadius = "ApoapsisRadius"
    PeriapsisRadius = "PeriapsisRadius"
    Cr = "Cr"
    Cd = "Cd"
    DryMass = "DryMass"
    PropMass = "PropMass"
    TotalMass = "TotalMass"
    # known to the reference, not available from a propagated ballistic state (StateError::Unavailable / NoThrusterAvail)
    Isp = "Isp"
    Thrust = "Thrust"


class StateError(Exception):
    """StateError::Unavailable { param } (cosmic/mod.rs)."""

    def __init__(self, param: StateParameter):
        super().__init__(f"{param.name} is unavailable for this state")
        self.param = param


_CART = {StateParameter.X: 0, StateParameter.Y: 1, StateParameter.Z: 2, StateParameter.VX: 3, StateParameter.VY: 4,
         StateParameter.VZ: 5}


def _wrap360(a):
    a = np.mod(a, 360.0)
    return np.where(a < 0.0, a + 360.0, a)


def state_value(param: StateParameter, rv: np.ndarray, mu_km3_s2: float, cr=None, cd=None, dry_mass_kg=None, prop_mass_kg=None,
                extra_mass_kg=None) -> np.ndarray:
    """Value of `param` for every row of `rv` ([..., 6], km and km/s).  Spacecraft-level parameters (Cr, Cd, masses)
    broadcast against the leading dimensions of `rv`; raises StateError for parameters a ballistic state does not have."""
    rv = np.asarray(rv, dtype=np.float64)
    lead = rv.shape[:-1]
    if param in _CART:
        return rv[..., _CART[param]].copy()
    sc = {StateParameter.Cr: cr, StateParameter.Cd: cd, StateParameter.DryMass: dry_mass_kg, StateParameter.PropMass: prop_mass_kg}
    if param in sc:
        if sc[param] is None:
            raise StateError(param)
        return np.broadcast_to(np.asarray(sc[param], dtype=np.float64), lead).copy()
    if param is StateParameter.TotalMass:
        if dry_mass_kg is None or prop_mass_kg is None:
            raise StateError(param)
        extra = 0.0 if extra_mass_kg is None else extra_mass_kg
        return np.broadcast_to(np.asarray(dry_mass_kg) + np.asarray(prop_mass_kg) + np.asarray(extra), lead).copy()
    if param in (StateParameter.Isp, StateParameter.Thrust):
        raise StateError(param)
    r, v = rv[..., :3], rv[..., 3:]
    rmag = np.linalg.norm(r, axis=-1)
    vmag = np.linalg.norm(v, axis=-1)
    if param is StateParameter.Rmag:
        return rmag
    if param is StateParameter.Vmag:
        return vmag
    h = np.cross(r, v)
    hmag = np.linalg.norm(h, axis=-1)
    if param is StateParameter.Hmag:
        return hmag
    energy = 0.5 * vmag * vmag - mu_km3_s2 / rmag
    if param is StateParameter.Energy:
        return energy
    sma = -mu_km3_s2 / (2.0 * energy)
    if param is StateParameter.SemiMajorAxis:
        return sma
    evec = ((vmag * vmag - mu_km3_s2 / rmag)[..., None] * r - np.sum(r * v, axis=-1)[..., None] * v) / mu_km3_s2
    ecc = np.linalg.norm(evec, axis=-1)
    if param is StateParameter.Eccentricity:
        return ecc
    if param is StateParameter.ApoapsisRadius:
        return sma * (1.0 + ecc)
    if param is StateParameter.PeriapsisRadius:
        return sma * (1.0 - ecc)
    if param is StateParameter.Period:
        return 2.0 * np.pi * np.sqrt(sma ** 3 / mu_km3_s2)
    if param is StateParameter.Inclination:
        return np.degrees(np.arccos(np.clip(h[..., 2] / hmag, -1.0, 1.0)))
    n = np.stack([-h[..., 1], h[..., 0], np.zeros_like(hmag)], axis=-1)  # z x h
    if param is StateParameter.RAAN:
        return _wrap360(np.degrees(np.arctan2(n[..., 1], n[..., 0])))
    if param is StateParameter.AoP:
        # angle from the node to the eccentricity vector, measured in the orbit plane around h
        cosw = np.sum(n * evec, axis=-1)
        sinw = np.sum(np.cross(n, evec) * h, axis=-1) / hmag
        return _wrap360(np.degrees(np.arctan2(sinw, cosw)))
    if param is StateParameter.TrueAnomaly:
        # atan2 form, as the device's event scalar (event_dev.h): well conditioned at the apsides
        cost = np.sum(evec * r, axis=-1)
        sint = np.sum(np.cross(evec, r) * h, axis=-1) / hmag
        return _wrap360(np.degrees(np.arctan2(sint, cost)))
    raise StateError(param)


def bplane_of_state(rv, mu_km3_s2: float):
    """(BdotT, BdotR) of every row of `rv` ([..., 6]) about a centre of `mu_km3_s2`: `bplane` on evec, ecc, h, hmag and sma exactly as
    `state_value` forms them."""
    rv = np.asarray(rv, dtype=np.float64)
    r, v = rv[..., :3], rv[..., 3:]
    with np.errstate(invalid="ignore", divide="ignore"):
        rmag = np.linalg.norm(r, axis=-1)
        vmag = np.linalg.norm(v, axis=-1)
        h = np.cross(r, v)
        hmag = np.linalg.norm(h, axis=-1)
        energy = 0.5 * vmag * vmag - mu_km3_s2 / rmag
        sma = -mu_km3_s2 / (2.0 * energy)
        evec = ((vmag * vmag - mu_km3_s2 / rmag)[..., None] * r - np.sum(r * v, axis=-1)[..., None] * v) / mu_km3_s2
        ecc = np.linalg.norm(evec, axis=-1)
    return bplane(evec, ecc, h, hmag, sma)


def bplane(evec, ecc, h, hmag, sma):
    """(BdotT, BdotR) of cosmic/bplane.rs:55-136 from the intermediates of `state_value`, NaN where ecc <= 1 (`BPlane::new`:
    NotHyperbolic).  e^ = evec / ecc, h^ = h / hmag, n^ = h^ x e^, f = sqrt(1 - (1 / ecc)(1 / ecc)); the incoming asymptote
    s = e^ / ecc + f n^; b = |sma| sqrt(ecc ecc - 1), the semi-minor axis; B = b (f e^ - (1 / ecc) n^); t = s^ x (0, 0, 1), r^ = s^ x t^.
    Sums of three as ((a0 + a1) + a2): the definition csrc/frame_dev.h (`frm_bplane`) restates operation for operation."""
    with np.errstate(invalid="ignore", divide="ignore"):
        inv_e = 1.0 / ecc
        eh, hh = evec / ecc[..., None], h / hmag[..., None]
        nh = _cross3(hh, eh)
        f = np.sqrt(1.0 - inv_e * inv_e)
        s = eh / ecc[..., None] + f[..., None] * nh
        sh = s / np.sqrt(_dot3(s, s))[..., None]
        b = np.abs(sma) * np.sqrt(ecc * ecc - 1.0)
        big_b = b[..., None] * (f[..., None] * eh - inv_e[..., None] * nh)
        t0, t1 = sh[..., 1], -sh[..., 0]                       # t = s^ x (0, 0, 1) = (s^_1, -s^_0, 0)
        tmag = np.sqrt(t0 * t0 + t1 * t1)
        th = np.stack([t0 / tmag, t1 / tmag, 0.0 / tmag], axis=-1)
        rh = _cross3(sh, th)
        hyp = ecc > 1.0
        return np.where(hyp, _dot3(big_b, th), np.nan), np.where(hyp, _dot3(big_b, rh), np.nan)


# ---- RIC differences (Traj::ric_diff_to_parquet, md/trajectory/traj.rs:407-600) ----
FRAME_OF = {"run": 0, "reference": 1, 0: 0, 1: 1}


def _dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross3(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def ric_difference(rv, rv_ref, frame_of="reference", transport=True) -> np.ndarray:
    """`rv - rv_ref` ([..., 6], km and km/s; the two broadcast) in the radial / in-track / cross-track frame of `rv`
    (`frame_of` "run" or 0: the reference's `self.ric_difference(&other)`) or of `rv_ref` ("reference" or 1: dispersions
    around a nominal): [dR, dI, dC, dvR, dvI, dvC].

    With d = rv - rv_ref (differenced first, component by component) and f the frame state: r^ = f_r / |f_r|, h = f_r x f_v,
    c^ = h / |h|, i^ = c^ x r^; the position and velocity differences are projected on (r^, i^, c^), and with `transport`
    the rotation rate of the frame, w = |h| / (|f_r| |f_r|) around c^, is removed from the velocity:
    dv = (dv_R + w dr_I, dv_I - w dr_R, dv_C) - a run that only lags the nominal on its circular orbit stands still.
    That term is the exact limit, under two-body motion, of the finite-differenced DCM rate ANISE applies
    (`Orbit::ric_difference`, `dcm_from_ric_to_inertial`); ANISE is not part of this reference tree, so like the other
    restatements here it follows the documented definition and is **parity unpinned**.

    Sums of three are taken as ((a0 + a1) + a2), as in `state_value`: this function is the definition the device kernel
    (csrc/ric_kernel.hip) restates operation for operation and is tested against bit for bit."""
    rv, rv_ref = np.broadcast_arrays(np.asarray(rv, dtype=np.float64), np.asarray(rv_ref, dtype=np.float64))
    if frame_of not in FRAME_OF:
        raise ValueError(f"ric_difference: frame_of must be 'run' / 0 or 'reference' / 1, not {frame_of!r}")
    d = rv - rv_ref
    f = rv_ref if FRAME_OF[frame_of] else rv
    fr, fv = f[..., :3], f[..., 3:]
    rmag = np.sqrt(_dot3(fr, fr))
    rhat = fr / rmag[..., None]
    h = _cross3(fr, fv)
    hmag = np.sqrt(_dot3(h, h))
    chat = h / hmag[..., None]
    ihat = _cross3(chat, rhat)
    dr, dv = d[..., :3], d[..., 3:]
    out = np.stack([_dot3(rhat, dr), _dot3(ihat, dr), _dot3(chat, dr), _dot3(rhat, dv), _dot3(ihat, dv), _dot3(chat, dv)], axis=-1)
    if transport:
        w = hmag / (rmag * rmag)
        vr = out[..., 3] + w * out[..., 1]
        vi = out[..., 4] - w * out[..., 0]
        out[..., 3], out[..., 4] = vr, vi
    return out


def smooth_ric(d, window: int = 5) -> np.ndarray:
    """`smooth_state_diff_in_place` (md/trajectory/mod.rs:75-125) on a copy of d[K, 6]: the median filter of the RIC
    differences.  k ascending and IN PLACE - the window [max(0, k - window / 2), min(K, k + window / 2 + 1)) of sample k holds
    the already smoothed samples before k -, the new value is element (end - start) / 2 of the sorted window, the six
    components independently.  Applied only when K > window (the reference smooths with 5 when it has more than 5
    samples, else with 1: the identity); an even window raises, as the reference asserts."""
    window = int(window)
    if window % 2 != 1 or window < 1:
        raise ValueError("smooth_ric: the window must be odd (median of the window)")
    out = np.array(d, dtype=np.float64)
    if out.ndim != 2 or out.shape[1] != 6:
        raise ValueError("smooth_ric: d must be [K, 6]")
    k_n, half = len(out), window // 2
    if k_n <= window:
        return out
    for k in range(k_n):
        start, end = max(0, k - half), min(k_n, k + half + 1)
        out[k] = np.sort(out[start:end], axis=0)[(end - start) // 2]
    return out
