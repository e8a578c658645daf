"""Ensemble statistics of a series report: THE DEFINITION (pure numpy + math, no GPU) of what `nyx_hip_series_stats` and
`nyx_hip_traj_series_stats` (include/nyx_hip_stats.h, csrc/stats_kernel.hip) leave per row and sample of a values block.

For row r and sample k of `values[R, K, n]` with `length[n]` and an optional `status[n]` (a run with status != 0 is left out, as
in nyx_hip_ensemble_moments): H the runs left in with k < min(length[i], K), C those of H whose value is not NaN, F those of C
whose value is finite.  The ten fixed columns are `Stat`; behind them one column per probability.

The total order is that of the IEEE bit pattern mapped to a monotone unsigned key (`total_order_key`): -inf < finite < +inf,
-0.0 before +0.0.  A quantile follows numpy's `linear` rule with a formula of its own, so that device and host round alike:
s = C sorted, m = |C|, h = (m - 1) * p, lo = floor(h), g = h - lo; s[lo] when g == 0 or s[lo] == s[lo + 1], else
s[lo] + g * (s[lo + 1] - s[lo]).  Every NaN a column holds (an empty C; -inf next to a larger value under the formula) is the
one quiet NaN of `math.nan`.  Mean and variance are derived: mean = SHIFT + SUM / FINITE, var = (SUMSQ - SUM^2 / FINITE) /
(FINITE - 1); SHIFT, the value of the first finite run, keeps the sums conditioned for |x| ~ 7000 km with 1 km dispersions.
"""
import math
from enum import IntEnum
from typing import NamedTuple, Optional, Sequence

import numpy as np

STAT_FIXED = 10
MAX_STAT_PROBS = 8


class Stat(IntEnum):
    """enum nyx_hip_stat: the values are part of the ABI."""
    HELD = 0
    COUNT = 1
    MIN = 2
    MAX = 3
    ARGMIN = 4
    ARGMAX = 5
    FINITE = 6
    SHIFT = 7
    SUM = 8
    SUMSQ = 9


class Request(NamedTuple):
    """What the `stats=` keyword of the `GpuContext.traj_*` reports takes besides a plain sequence of probabilities: the
    probabilities and the status of every run (a run with status != 0 is left out of the statistics)."""
    probs: Sequence[float] = ()
    status: Optional[Sequence[int]] = None


def request(stats) -> "Request":
    """`stats=` as a Request: a Request as it is, anything else a sequence of probabilities."""
    return stats if isinstance(stats, Request) else Request(tuple(stats), None)


def total_order_key(v) -> np.ndarray:
    """uint64 keys whose unsigned order is the total order of the doubles `v` (stat_key of csrc/stats_dev.h)."""
    bits = np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)
    return np.where(bits >> np.uint64(63), ~bits, bits | np.uint64(1 << 63))


def check_probs(probs) -> np.ndarray:
    p = np.asarray(list(probs), dtype=np.float64).reshape(-1)
    if len(p) > MAX_STAT_PROBS:
        raise ValueError(f"series_stats: {len(p)} probabilities, 0 .. {MAX_STAT_PROBS} per call")
    if not np.all((p >= 0.0) & (p <= 1.0)):   # (a NaN fails both)
        raise ValueError("series_stats: every probability must lie in [0, 1]")
    return p


def quantile_of_sorted(s: np.ndarray, p: float) -> float:
    """The quantile `p` of `s`, sorted in the total order and free of NaN (stat_quantile of csrc/stats_dev.h)."""
    m = len(s)
    if m == 0:
        return math.nan
    h = float(m - 1) * float(p)
    lo = math.floor(h)
    g = h - lo
    a = float(s[lo])
    if g == 0.0:
        return a
    b = float(s[lo + 1])
    if a == b:
        return a
    q = a + g * (b - a)
    return math.nan if q != q else q


def sample_stats(v: np.ndarray, runs: np.ndarray, probs) -> np.ndarray:
    """The columns of one (row, sample): `v` the values of the runs of H, `runs` their indices, ascending."""
    out = np.empty(STAT_FIXED + len(probs))
    c = ~np.isnan(v)
    vc, ic = v[c], runs[c]
    out[Stat.HELD], out[Stat.COUNT] = len(v), len(vc)
    if len(vc):
        key = total_order_key(vc)
        order = np.argsort(key, kind="stable")
        s = vc[order]
        out[Stat.MIN], out[Stat.MAX] = s[0], s[-1]
        out[Stat.ARGMIN], out[Stat.ARGMAX] = ic[key == key[order[0]]][0], ic[key == key[order[-1]]][0]
    else:
        s = vc
        out[Stat.MIN] = out[Stat.MAX] = math.nan
        out[Stat.ARGMIN] = out[Stat.ARGMAX] = -1.0
    f = vc[np.isfinite(vc)]
    out[Stat.FINITE] = len(f)
    shift = float(f[0]) if len(f) else 0.0
    d = f - shift
    out[Stat.SHIFT], out[Stat.SUM], out[Stat.SUMSQ] = shift, math.fsum(d), math.fsum(d * d)
    for j, p in enumerate(probs):
        out[STAT_FIXED + j] = quantile_of_sorted(s, p)
    return out


def series_stats(values, length, probs=(), status=None) -> np.ndarray:
    """stats[R, K, 10 + len(probs)] of `values[R, K, n]` (K = the capacity), `length[n]` and the optional `status[n]`."""
    values = np.asarray(values, dtype=np.float64)
    if values.ndim != 3:
        raise ValueError("series_stats: values must be [rows, capacity, n]")
    rows, cap, n = values.shape
    length = np.asarray(length).reshape(-1)
    if len(length) != n or (status is not None and len(np.asarray(status).reshape(-1)) != n):
        raise ValueError("series_stats: length and status hold one entry per run")
    probs = check_probs(probs)
    keep = np.ones(n, dtype=bool) if status is None else np.asarray(status).reshape(-1) == 0
    out = np.empty((rows, cap, STAT_FIXED + len(probs)))
    for k in range(cap):
        held = keep & (k < np.minimum(length, cap))
        runs = np.nonzero(held)[0]
        for r in range(rows):
            out[r, k] = sample_stats(values[r, k, held], runs, probs)
    return out


class SeriesStats:
    """The statistics of a report: `stats[R, K, 10 + P]`, what its rows are, the probabilities, and the samples' epochs where the
    report has one grid for all runs."""

    def __init__(self, stats: np.ndarray, rows, probs, step_ns=None, epoch0_ns=None):
        self.stats = np.asarray(stats)
        self.rows = list(rows)
        self.probs = tuple(float(p) for p in probs)
        self.step_ns, self.epoch0_ns = step_ns, epoch0_ns
        if self.stats.ndim != 3 or self.stats.shape[0] != len(self.rows) or self.stats.shape[2] != STAT_FIXED + len(self.probs):
            raise ValueError("SeriesStats: stats must be [len(rows), capacity, 10 + len(probs)]")

    def of(self, stat) -> np.ndarray:
        """[R, K]: one fixed column."""
        return self.stats[:, :, int(Stat(stat))]

    def quantile(self, j: int) -> np.ndarray:
        """[R, K]: the quantile probs[j]."""
        if not 0 <= j < len(self.probs):
            raise IndexError(f"quantile {j} of {len(self.probs)}")
        return self.stats[:, :, STAT_FIXED + j]

    def mean(self) -> np.ndarray:
        """[R, K] over the finite values; NaN where there is none."""
        n = self.of(Stat.FINITE)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(n > 0, self.of(Stat.SHIFT) + self.of(Stat.SUM) / n, np.nan)

    def var(self) -> np.ndarray:
        """[R, K] sample variance (n - 1) over the finite values; NaN with fewer than two."""
        n, s = self.of(Stat.FINITE), self.of(Stat.SUM)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(n > 1, (self.of(Stat.SUMSQ) - s * s / n) / (n - 1), np.nan)

    def std(self) -> np.ndarray:
        return np.sqrt(self.var())

    def epochs(self) -> np.ndarray:
        """int64[K]: the epoch of every sample, where a first epoch is known."""
        if self.step_ns is None or self.epoch0_ns is None:
            raise ValueError("SeriesStats.epochs: the report has no common first epoch")
        return int(self.epoch0_ns) + np.arange(self.stats.shape[1], dtype=np.int64) * int(self.step_ns)
