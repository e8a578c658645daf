"""Blocks of values for the statistics tests (tests/test_stats_host.py, tests/test_stats_host_cxx.py, tests/test_gpu_stats.py): one
maker, seeded, so that the CPU definition, the host build of csrc/stats_dev.h and the device see the same adversarial patterns."""
import numpy as np

PROBS = (0.0, 0.01, 0.25, 0.5, 0.75, 0.99, 1.0)


def integral_prob(m: int) -> float:
    """A probability strictly inside (0, 1) with (m - 1) * p an integer in double arithmetic (m >= 3); 0.5 otherwise."""
    for j in range(1, m - 1):
        p = j / (m - 1)
        if float(m - 1) * p == float(j):
            return p
    return 0.5


def held_count(length, cap: int, k: int, status=None) -> int:
    """|H| of sample k: the m of a sample without NaN."""
    keep = np.ones(len(length), dtype=bool) if status is None else np.asarray(status) == 0
    return int((keep & (k < np.minimum(length, cap))).sum())


def block_probs(length, cap: int, k: int, status=None):
    """PROBS plus one probability with (m - 1) * p integral for the m of sample k (the tie sample of a block: no NaN there)."""
    return PROBS + (integral_prob(held_count(length, cap, k, status)),)


def adversarial_block(n: int, rows: int = 3, cap: int = 5, seed: int = 0):
    """(values[rows, cap, n], length[n] int32, status[n] int32): normal data around 7000 with unit dispersion, then per sample k
    of every row one pattern: 0 NaN sprinkled, 1 a row that is all NaN, 2 +-inf sprinkled (and -0.0 against +0.0 in row 1), 3 all
    values equal, 4 ties and signed zeros.  `length` holds 0, values above the capacity and everything between; `status` removes
    runs, the smallest-index one among them when n > 1."""
    rng = np.random.default_rng(1000 * seed + n)
    v = 7000.0 + rng.standard_normal((rows, cap, n))
    for r in range(rows):
        k = 0
        v[r, k % cap, rng.random(n) < 0.3] = np.nan
        k = 1
        v[r, k % cap, :] = np.nan
        k = 2
        hit = rng.random(n)
        v[r, k % cap, hit < 0.2] = np.inf
        v[r, k % cap, hit > 0.8] = -np.inf
        if r == 1:
            v[r, k % cap, :] = np.where(rng.random(n) < 0.5, 0.0, -0.0)
        k = 3
        v[r, k % cap, :] = 6999.5 + r
        k = 4
        v[r, k % cap, :] = np.round(rng.standard_normal(n))      # many ties, +0.0 and -0.0 (a rounded small negative is -0.0)
    length = rng.integers(0, cap + 3, size=n).astype(np.int32)
    if n >= 3:
        length[0], length[1], length[2] = cap + 2, 0, cap
    else:
        length[:] = cap
    status = (rng.random(n) < 0.15).astype(np.int32)
    if n > 1:
        status[0] = 1                                            # SHIFT and ARGMIN must react to the first run leaving
    return v, length, status


def big_block(n: int, seed: int = 7):
    """A 1 x 2 block for the sizes around the LDS limit: sample 0 normal data with NaN and inf sprinkled, sample 1 heavy ties."""
    rng = np.random.default_rng(seed + n)
    v = np.empty((1, 2, n))
    v[0, 0] = 7000.0 + rng.standard_normal(n)
    hit = rng.random(n)
    v[0, 0, hit < 0.01] = np.nan
    v[0, 0, hit > 0.995] = np.inf
    v[0, 1] = rng.integers(-3, 4, size=n).astype(np.float64)
    length = np.full(n, 2, dtype=np.int32)
    length[rng.random(n) < 0.05] = 1
    status = (rng.random(n) < 0.02).astype(np.int32)
    return v, length, status


def canonical_bits(a) -> np.ndarray:
    """The bit patterns of `a` (every NaN the library writes is 0x7FF8000000000000, as numpy's nan)."""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def compare(got: np.ndarray, want: np.ndarray, values, length, status, label: str = ""):
    """`got` against the definition `want` by the tolerances of the statistics: everything bit for bit but SUM within
    FINITE * 2^-53 * sum |d| and SUMSQ within FINITE * 2^-53 * sum d^2 of the fsum value (the classical bound of any order)."""
    from nyx_amd.stats import STAT_FIXED, Stat
    assert got.shape == want.shape, (label, got.shape, want.shape)
    exact = [s for s in range(want.shape[2]) if s not in (Stat.SUM, Stat.SUMSQ)]
    gb, wb = canonical_bits(got), canonical_bits(want)
    bad = np.argwhere(gb[:, :, exact] != wb[:, :, exact])
    assert len(bad) == 0, (label, [(tuple(b), got[b[0], b[1], exact[b[2]]], want[b[0], b[1], exact[b[2]]]) for b in bad[:5]])
    rows, cap, n = values.shape
    keep = np.ones(n, dtype=bool) if status is None else np.asarray(status) == 0
    u = 2.0 ** -53
    for k in range(cap):
        held = keep & (k < np.minimum(length, cap))
        for r in range(rows):
            x = values[r, k, held]
            f = x[np.isfinite(x)]
            d = f - want[r, k, Stat.SHIFT]
            bound1, bound2 = len(f) * u * np.abs(d).sum(), len(f) * u * (d * d).sum()
            e1, e2 = abs(got[r, k, Stat.SUM] - want[r, k, Stat.SUM]), abs(got[r, k, Stat.SUMSQ] - want[r, k, Stat.SUMSQ])
            assert e1 <= bound1 and e2 <= bound2, (label, r, k, e1, bound1, e2, bound2)
    assert STAT_FIXED == 10
