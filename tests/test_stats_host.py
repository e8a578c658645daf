"""CPU: the definition of the ensemble statistics (nyx_amd/stats.py) against a brute-force evaluation per (row, sample) that
shares nothing with it but the words of include/nyx_hip_stats.h: Python's sort on an integer key made with `struct`, explicit
loops, `math.fsum`.  Quantiles on finite data are also held to numpy's own `linear` rule within
4 x spacing(max(|s[lo]|, |s[lo + 1]|)): each of the two formulas rounds three times."""
import math
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from stats_cases import adversarial_block, block_probs, canonical_bits, held_count, integral_prob  # noqa: E402

from nyx_amd import stats as st  # noqa: E402
from nyx_amd.stats import STAT_FIXED, Stat  # noqa: E402


def brute_key(x: float) -> int:
    b = struct.unpack("<Q", struct.pack("<d", x))[0]
    return (~b) & 0xFFFFFFFFFFFFFFFF if b >> 63 else b | (1 << 63)


def brute(values, length, probs, status):
    rows, cap, n = values.shape
    out = np.empty((rows, cap, STAT_FIXED + len(probs)))
    for r in range(rows):
        for k in range(cap):
            h = [i for i in range(n) if (status is None or status[i] == 0) and k < min(int(length[i]), cap)]
            c = [i for i in h if not math.isnan(values[r, k, i])]
            f = [i for i in c if math.isfinite(values[r, k, i])]
            o = out[r, k]
            o[0], o[1], o[6] = len(h), len(c), len(f)
            s = sorted(c, key=lambda i: (brute_key(values[r, k, i]), i))
            if c:
                o[2], o[3] = values[r, k, s[0]], values[r, k, s[-1]]
                o[4] = s[0]
                o[5] = min(i for i in c if brute_key(values[r, k, i]) == brute_key(values[r, k, s[-1]]))
            else:
                o[2] = o[3] = math.nan
                o[4] = o[5] = -1
            shift = values[r, k, f[0]] if f else 0.0
            d = [values[r, k, i] - shift for i in f]
            o[7], o[8], o[9] = shift, math.fsum(d), math.fsum(x * x for x in d)
            for j, p in enumerate(probs):
                if not c:
                    o[10 + j] = math.nan
                    continue
                hh = (len(c) - 1) * p
                lo = int(math.floor(hh))
                g = hh - lo
                a = float(values[r, k, s[lo]])
                if g == 0 or a == values[r, k, s[lo + 1]]:
                    o[10 + j] = a
                else:
                    q = a + g * (float(values[r, k, s[lo + 1]]) - a)
                    o[10 + j] = math.nan if math.isnan(q) else q
    return out


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257])
def test_the_definition_agrees_with_brute_force_on_every_pattern(n):
    v, length, status = adversarial_block(n)
    probs = block_probs(length, 5, 4)
    m = held_count(length, 5, 4)
    assert m < 3 or (0.0 < probs[-1] < 1.0 and float(m - 1) * probs[-1] == round(float(m - 1) * probs[-1]))     # an interior integral rank at the tie sample
    for stt in (None, status):
        got, want = st.series_stats(v, length, probs, status=stt), brute(v, length, probs, stt)
        assert (canonical_bits(got) == canonical_bits(want)).all(), np.argwhere(canonical_bits(got) != canonical_bits(want))[:5]


def test_extremes_orders_and_the_bracket_of_a_quantile():
    v, length, status = adversarial_block(65)
    probs = block_probs(length, 5, 4, status)
    got = st.series_stats(v, length, probs, status=status)
    bits = canonical_bits(got)
    assert (bits[:, :, 10] == bits[:, :, Stat.MIN]).all() and (bits[:, :, 16] == bits[:, :, Stat.MAX]).all()      # p = 0 / 1
    keep = status == 0
    for r in range(v.shape[0]):
        for k in range(v.shape[1]):
            x = v[r, k, keep & (k < np.minimum(length, v.shape[1]))]
            x = x[~np.isnan(x)]
            s = x[np.argsort(st.total_order_key(x), kind="stable")]
            for j, p in enumerate(probs):
                q = got[r, k, 10 + j]
                if len(s) == 0:
                    assert math.isnan(q)
                    continue
                h = (len(s) - 1) * p
                lo = math.floor(h)
                if h == lo:
                    assert canonical_bits(q) == canonical_bits(s[lo])                       # an order statistic, exactly
                elif not math.isnan(q):
                    assert s[lo] <= q <= s[lo + 1]
                else:
                    assert math.isinf(s[lo]) and s[lo] < 0 and s[lo + 1] > s[lo]          # -inf beside a larger value: the formula's NaN


def test_quantiles_of_finite_data_are_numpys_linear_rule():
    rng = np.random.default_rng(5)
    for m in (1, 2, 3, 10, 101, 1000, 10000):
        x = 7000.0 + rng.standard_normal(m)
        probs = (0.0, 0.01, 0.25, 0.5, 0.75, 0.99, 1.0, integral_prob(m))
        got = st.series_stats(x.reshape(1, 1, m), np.ones(m, dtype=np.int32), probs)[0, 0, 10:]
        s = np.sort(x)
        for q, p in zip(got, probs):
            lo = int(math.floor((m - 1) * p))
            scale = max(abs(s[lo]), abs(s[min(lo + 1, m - 1)]))
            assert abs(q - np.quantile(x, p, method="linear")) <= 4 * np.spacing(scale), (m, p)


def test_infinities_count_but_stay_out_of_the_sums_and_signed_zeros_are_ordered():
    v = np.array([[[np.inf, 1.0, -np.inf, 3.0, np.nan, np.inf]]])
    got = st.series_stats(v, np.ones(6, dtype=np.int32), (0.0, 1.0, 0.5))[0, 0]
    assert got[Stat.HELD] == 6 and got[Stat.COUNT] == 5 and got[Stat.FINITE] == 2
    assert got[Stat.MIN] == -np.inf and got[Stat.MAX] == np.inf and got[Stat.ARGMIN] == 2 and got[Stat.ARGMAX] == 0
    assert got[Stat.SHIFT] == 1.0 and got[Stat.SUM] == 2.0 and got[Stat.SUMSQ] == 4.0
    assert got[10] == -np.inf and got[11] == np.inf and got[12] == 3.0
    two = st.series_stats(np.array([[[np.inf, np.inf, np.inf]]]), np.ones(3, dtype=np.int32), (0.25,))[0, 0]
    assert two[10] == np.inf and two[Stat.FINITE] == 0 and two[Stat.SHIFT] == 0.0                    # never inf - inf
    z = st.series_stats(np.array([[[0.0, -0.0, 0.0, -0.0]]]), np.ones(4, dtype=np.int32), (0.0, 1.0))[0, 0]
    assert math.copysign(1.0, z[Stat.MIN]) == -1.0 and math.copysign(1.0, z[Stat.MAX]) == 1.0
    assert z[Stat.ARGMIN] == 1 and z[Stat.ARGMAX] == 0


def test_status_len_and_capacity_decide_who_is_held():
    v = np.arange(12, dtype=np.float64).reshape(1, 3, 4)           # sample k of run i = 4 k + i
    length = np.array([5, 0, 2, 3], dtype=np.int32)                  # above the capacity, none, two, all
    got = st.series_stats(v, length, (0.5,))
    assert got[0, :, Stat.HELD].tolist() == [3, 3, 2]
    assert got[0, :, Stat.ARGMIN].tolist() == [0, 0, 0] and got[0, :, Stat.SHIFT].tolist() == [0.0, 4.0, 8.0]
    out = st.series_stats(v, length, (0.5,), status=np.array([1, 0, 0, 0], dtype=np.int32))          # the smallest-index run leaves
    assert out[0, :, Stat.HELD].tolist() == [2, 2, 1]
    assert out[0, :, Stat.ARGMIN].tolist() == [2, 2, 3] and out[0, :, Stat.SHIFT].tolist() == [2.0, 6.0, 11.0]
    empty = st.series_stats(np.zeros((2, 3, 0)), np.zeros(0, dtype=np.int32), (0.5,))
    assert empty.shape == (2, 3, 11) and (empty[:, :, [0, 1, 6, 7, 8, 9]] == 0).all() and (empty[:, :, [4, 5]] == -1).all()
    assert np.isnan(empty[:, :, [2, 3, 10]]).all()


def test_mean_and_sigma_are_conditioned_by_the_shift():
    rng = np.random.default_rng(2)
    x = 7000.0 + rng.standard_normal(10000)
    s = st.SeriesStats(st.series_stats(x.reshape(1, 1, -1), np.ones(10000, dtype=np.int32), (0.5,)), ["x"], (0.5,), step_ns=10, epoch0_ns=5)
    # (the mean: a few roundings at 7000 on either side, 4 ulp; sigma ~ 1 from two well-conditioned sums: 1e-12 is four digits above either error)
    assert abs(s.mean()[0, 0] - math.fsum(x) / 10000) <= 4 * np.spacing(7000.0) and abs(s.std()[0, 0] - np.std(x, ddof=1)) < 1e-12
    assert s.of(Stat.COUNT)[0, 0] == 10000 and s.quantile(0)[0, 0] == np.quantile(x, 0.5) and s.epochs().tolist() == [5]
    assert s.rows == ["x"] and s.probs == (0.5,)


def test_probabilities_are_refused_as_the_library_refuses_them():
    one = np.zeros((1, 1, 1)), np.ones(1, dtype=np.int32)
    for bad in ((-0.1,), (1.5,), (math.nan,), tuple([0.5] * 9)):
        with pytest.raises(ValueError):
            st.series_stats(*one, bad)
