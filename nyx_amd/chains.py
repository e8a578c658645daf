"""The ephemeris chain: [(segment, sign), ...], whose signed sum of the almanac's Chebyshev (SPK type 2) segments, in chain order and
from zero, is a body's state about the integration centre.  What the eclipse, encounter, link, Lambert and targeter modules share:
the chain of a body, what a chain is refused for, its copy into a query struct, and its evaluation.

The evaluation restates the oracle's `cheby_eval` / `cheby_eval_pv` / `body_position` / `frame_shift` (oracle/nyx_oracle.c) OPERATION
FOR OPERATION - the rolled Clenshaw recurrence with its companion derivative, one rounding per operation, sums along the chain in
chain order - so that it agrees with the oracle, and the device kernels (csrc/chain_dev.h) with it, bit for bit.  An epoch outside a
segment gives NaN (the range rule: beyond the last record only the end of coverage itself is inside).
"""
from __future__ import annotations

import numpy as np

from ._abi import MAX_CHAIN


def body_chain(naif_id: int, almanac, central):
    """[(segment, sign), ...] of a body w.r.t. `central` in `almanac`; [] for the central body itself."""
    if int(naif_id) == int(central.naif_id):
        return []
    if naif_id not in almanac.bodies:
        raise KeyError(f"planetary data of body {naif_id} not loaded")
    return [(int(s), int(g)) for s, g in almanac.bodies[naif_id]["chain"]]


def checked_chain(chain, almanac, subject: str, least: int = 0, note: str = ""):
    """`chain`, refusing what `check_chain` (csrc/chain_args.h) refuses, in its order: ValueError, worded about `subject`."""
    if not least <= len(chain) <= MAX_CHAIN:
        raise ValueError(f"{subject} has a chain of {len(chain)} segments, {least} .. {MAX_CHAIN}{note}")
    for seg, sign in chain:
        if not 0 <= seg < len(almanac.segments):
            raise ValueError(f"{subject} names segment {seg}, not a segment of the almanac")
        if sign not in (1, -1):
            raise ValueError(f"{subject} has a chain sign {sign}, +1 or -1")
    return chain


def fill_chain(dst, chain) -> None:
    """`chain` into the n_chain / chain_segment / chain_sign of a query struct of _abi.py."""
    dst.n_chain = len(chain)
    for k, (seg, sign) in enumerate(chain):
        dst.chain_segment[k], dst.chain_sign[k] = seg, sign


def cheby_state(seg, et_s, with_v: bool = True):
    """`cheby_eval_pv` of oracle/nyx_oracle.c for an array of epochs: (r[..., 3], v[..., 3]); NaN where et lies outside the segment.
    The value by the Clenshaw recurrence, the derivative by its companion, scaled by 1 / radius; without `with_v` the companion is
    not run and v is None."""
    et = np.asarray(et_s, dtype=np.float64)
    rec_all = np.asarray(seg.records, dtype=np.float64)
    n_rec, nc = rec_all.shape[0], seg.n_coeffs
    with np.errstate(invalid="ignore"):
        idx = np.floor((et - float(seg.init_et_s)) / float(seg.interval_s))
        end = float(seg.init_et_s) + float(seg.interval_s) * float(n_rec)
        bad = ~(idx >= 0) | (idx > n_rec) | ((idx == n_rec) & (et > end))
    idx = np.where(bad, 0, np.minimum(np.where(bad, 0, idx), n_rec - 1)).astype(np.int64)   # (idx == n_rec: exactly the end of coverage)
    rec = rec_all[idx]
    t = (et - rec[..., 0]) / rec[..., 1]
    two_t = 2.0 * t
    r, v = np.empty(et.shape + (3,)), np.empty(et.shape + (3,)) if with_v else None
    for c in range(3):
        cf = rec[..., 2 + c * nc:2 + (c + 1) * nc]
        w0, w1, d0, d1 = np.zeros(et.shape), np.zeros(et.shape), np.zeros(et.shape), np.zeros(et.shape)
        for j in range(nc - 1, 0, -1):
            w2 = w1
            w1 = w0
            w0 = cf[..., j] + (two_t * w1 - w2)
            if with_v:
                d2 = d1
                d1 = d0
                d0 = (2.0 * w1 + two_t * d1) - d2
        r[..., c] = cf[..., 0] + (t * w0 - w1)
        if with_v:
            v[..., c] = ((w0 + t * d0) - d1) / rec[..., 1]
    r[bad] = np.nan
    if with_v:
        v[bad] = np.nan
    return r, v


def cheby_position(seg, et_s) -> np.ndarray:
    """`cheby_eval` of oracle/nyx_oracle.c for an array of epochs: [..., 3], the position half of `cheby_state`."""
    return cheby_state(seg, et_s, with_v=False)[0]


def chain_state(chain, et_s, almanac, with_v: bool = True):
    """The signed sum of a chain at the epochs `et_s` (seconds), in chain order, from zero: (r[..., 3], v[..., 3], inside[...]);
    v is None without `with_v`.  An empty chain is the centre itself: zeros, inside everywhere."""
    et = np.asarray(et_s, dtype=np.float64)
    r, v = np.zeros(et.shape + (3,)), np.zeros(et.shape + (3,)) if with_v else None
    inside = np.ones(et.shape, dtype=bool)
    for seg, sign in chain:
        p, pv = cheby_state(almanac.segments[seg], et, with_v)
        inside &= ~np.isnan(p[..., 0])
        r = r + float(sign) * p
        if with_v:
            v = v + float(sign) * pv
    return r, v, inside
