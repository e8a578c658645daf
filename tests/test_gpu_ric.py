"""Fused RIC dispersions (ric_kernel.hip, include/nyx_hip_ric.h) on the MI355X.

The two interpolated states a difference is formed from are the ones `traj_every` / `traj_at` return (same device code), and
the difference itself is +, -, x, / and sqrt in the order of `nyx_amd.params.ric_difference`, compiled without contraction:
with `smooth_window=0` the device must agree with that host function applied to the `traj_every` states BIT FOR BIT.  The
median filter selects, the moments are held to the worst-case bound of ANY summation order.  Small on purpose: a few
hundred trajectories, hours, 8x8 gravity.

TOLERANCES (test 1).  Measured on the MI355X (256 dispersed LEO trajectories, e = 0.05, i = 68.5 deg, 3 h, one sample per
60 s = 46 336 samples per component, both frames, with and without the transport term, one nominal and pairwise): the
largest |device - ric_difference| per component.  A bound would be the measured figure x 8 rounded up to one significant
digit, never above the ceilings 1e-12 km / 1e-15 km/s; a measured 0 stays 0: those are exact.

    component   measured   unit   bound
    dR          0          km     0
    dI          0          km     0
    dC          0          km     0
    dvR         0          km/s   0
    dvI         0          km/s   0
    dvC         0          km/s   0
"""
import copy
import ctypes as C
import dataclasses
import math

import numpy as np
import pytest

import nyx_amd as nx
from nyx_amd import _abi
from nyx_amd import ephem
from nyx_amd.params import ric_difference, smooth_ric
from scenarios import EARTH_RADIUS_KM, EPOCH0_NS, dispersed_leo_batch, keplerian_to_cartesian, leo_full_setup, leo_nominal

pytestmark = pytest.mark.gpu

S = nx.NS_PER_S
STEP = 60 * S
NAMES = ["dR", "dI", "dC", "dvR", "dvI", "dvC"]
CEILING = [1e-12] * 3 + [1e-15] * 3
TOL = [0.0, 0.0, 0.0, 0.0, 0.0, 0.0]        # see the table above
IU = np.triu_indices(6)


def assert_within(got, want, what=""):
    """got, want: [..., 6]; prints the largest deviation of every component before it asserts."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and np.isfinite(want).all() and np.isfinite(got).all(), what
    failures = []
    for c in range(6):
        d = float(np.abs(got[..., c] - want[..., c]).max()) if got.size else 0.0
        print(f"deviation {what:36s} {NAMES[c]:4s} {d:.3e}  (bound {TOL[c]:.0e})")
        assert TOL[c] <= CEILING[c]
        if d > TOL[c]:
            failures.append(f"{what} {NAMES[c]}: {d:.3e} > {TOL[c]:.0e}")
    assert not failures, "\n".join(failures)


def assert_moments_within_the_summation_bound(mom, d):
    """Every sum of n terms, in whatever order, lies within gamma_n sum|term| of the exact sum, gamma_n = n u / (1 - n u),
    u = 2^-53; math.fsum is the exact sum, rounded once.  d: [n, 6], the columns that have the sample."""
    n = len(d)
    u = 2.0 ** -53
    gamma = n * u / (1.0 - n * u)
    assert mom[0] == n                                                      # counts are exact
    terms = [d[:, c] for c in range(6)] + [d[:, r] * d[:, c] for r, c in zip(*IU)]
    for q, t in enumerate(terms):
        exact = math.fsum(t.tolist())
        bound = gamma * math.fsum(np.abs(t).tolist()) + u * abs(exact)
        assert abs(mom[1 + q] - exact) <= bound, (q, mom[1 + q], exact, bound)


@pytest.fixture(scope="module")
def leo():
    prop, almanac, central = leo_full_setup(degree=8)
    compiled = prop.compile(almanac, central)
    ctx = nx.GpuContext(compiled)
    yield prop, almanac, central, compiled, ctx
    ctx.close()


NOMINAL = keplerian_to_cartesian((EARTH_RADIUS_KM + 300.0) / 0.95, 0.05, 68.5, 65.2, 75.0, 0.0, ephem.MU_EARTH)


def _nominal_batch():
    b = dispersed_leo_batch(1, seed=0, nominal=NOMINAL)
    b.set_rv(NOMINAL[None, :])
    return b


@pytest.fixture(scope="module")
def leo256(leo):
    """(runs, one nominal, 256 other trajectories for the pairwise case), 3 h each."""
    ctx = leo[4]
    out, st, traj = ctx.propagate_with_traj(dispersed_leo_batch(256, seed=11, nominal=NOMINAL), 3 * 3600 * S, capacity=400)
    assert (st.status == 0).all()
    _, st1, nom = ctx.propagate_with_traj(_nominal_batch(), 3 * 3600 * S, capacity=400)
    _, st2, pair = ctx.propagate_with_traj(dispersed_leo_batch(256, seed=12, nominal=NOMINAL), 3 * 3600 * S, capacity=400)
    assert (st1.status == 0).all() and (st2.status == 0).all()
    return traj, nom, pair


def every_states(ctx, traj, step, cap):
    """states[K, n, 6] of traj_every."""
    ev = ctx.traj_every(traj, step, cap)
    return np.ascontiguousarray(ev.state.transpose(1, 2, 0)), ev.len


def expected_series(traj, ref, step, start=None, end=None):
    lo, hi = nx.ric_bounds(traj, ref, start, end)
    return lo, np.where(hi >= lo, (hi - lo) // step + 1, 0)


def test_1_unsmoothed_values_are_ric_difference_of_the_traj_every_states(leo, leo256):
    ctx = leo[4]
    traj, nom, pair = leo256
    rv, ln = every_states(ctx, traj, STEP, 181)
    assert (ln == 181).all()
    failures = []
    for ref in (nom, pair):
        rr, rl = every_states(ctx, ref, STEP, 181)
        assert (rl == 181).all()
        lo, count = expected_series(traj, ref, STEP)
        for frame_of in ("run", "reference"):
            for transport in (True, False):
                vals, length, epoch0, mom = ctx.traj_ric_diff(traj, ref, STEP, capacity=181, frame_of=frame_of, transport=transport, smooth_window=0)
                assert vals.shape == (6, 181, 256) and length.dtype == np.int32 and epoch0.dtype == np.int64 and mom is None
                np.testing.assert_array_equal(length, count)
                np.testing.assert_array_equal(epoch0, lo)
                assert (length == 181).all() and (epoch0 == EPOCH0_NS).all()
                want = ric_difference(rv, rr, frame_of=frame_of, transport=transport)       # [181, 256, 6]; one nominal broadcasts
                try:
                    assert_within(vals.transpose(1, 2, 0), want, f"n_ref={ref.n} frame={frame_of} transport={transport}")
                except AssertionError as e:
                    failures.append(str(e))
    assert not failures, "\n".join(failures)
    # ~1 km dispersions that grow along the track: the numbers are dispersions
    assert 0.1 < np.abs(vals[:3, 0]).max() < 15.0 and np.abs(vals[1, 180]).max() > np.abs(vals[1, 0]).max()
    # capacity=None: sized from the epochs of the two batches; the integer 0 / 1 spelling of the frame
    v2, l2, e2, _ = ctx.traj_ric_diff(traj, pair, STEP, frame_of=1, transport=False, smooth_window=0)
    assert v2.shape == (6, 181, 256)
    np.testing.assert_array_equal(v2, vals)
    np.testing.assert_array_equal(l2, length)
    # a step that does not divide the span and a ragged last chunk, in a window that starts inside
    step, start, stop = 47 * S + 13, EPOCH0_NS + 1000 * S + 7, EPOCH0_NS + 9000 * S
    vals, length, epoch0, _ = ctx.traj_ric_diff(traj, nom, step, start, stop, capacity=200, smooth_window=0)
    lo, count = expected_series(traj, nom, step, start, stop)
    np.testing.assert_array_equal(length, count)
    np.testing.assert_array_equal(epoch0, lo)
    k_n = int(count[0])
    assert (count == k_n).all() and (lo == start).all() and 160 < k_n < 200
    q = start + step * np.arange(k_n)
    a, sa = ctx.traj_at(traj, q)
    b, sb = ctx.traj_at(nom, q)
    assert not _abi.interp_failed(sa).any() and not _abi.interp_failed(sb).any()
    assert_within(vals[:, :k_n].transpose(1, 2, 0), ric_difference(a, b), "windowed, odd step")
    assert np.isnan(vals[:, k_n:]).all()


def test_2_the_median_filter_is_smooth_ric_of_the_unsmoothed_output(leo, leo256):
    ctx = leo[4]
    traj, nom, _ = leo256
    raw, length, _, _ = ctx.traj_ric_diff(traj, nom, STEP, capacity=181, smooth_window=0)
    same, _, _, _ = ctx.traj_ric_diff(traj, nom, STEP, capacity=181, smooth_window=1)
    np.testing.assert_array_equal(same, raw)
    for window, runs in ((5, range(256)), (3, range(0, 256, 9)), (7, range(1, 256, 9)), (9, range(2, 256, 9))):
        got, l2, _, _ = ctx.traj_ric_diff(traj, nom, STEP, capacity=181, smooth_window=window)
        np.testing.assert_array_equal(l2, length)
        assert not np.array_equal(got, raw)
        for i in runs:
            np.testing.assert_array_equal(got[:, :, i], smooth_ric(raw[:, :, i].T, window).T, err_msg=f"window {window}, run {i}")
    # no more samples than the window: untouched (the reference filters with 5 only when it has more than 5 samples)
    end6, end5 = EPOCH0_NS + 5 * STEP, EPOCH0_NS + 4 * STEP
    r6, l6, _, _ = ctx.traj_ric_diff(traj, nom, STEP, EPOCH0_NS, end6, smooth_window=0)
    s6, _, _, _ = ctx.traj_ric_diff(traj, nom, STEP, EPOCH0_NS, end6, smooth_window=5)
    r5, l5, _, _ = ctx.traj_ric_diff(traj, nom, STEP, EPOCH0_NS, end5, smooth_window=0)
    s5, _, _, _ = ctx.traj_ric_diff(traj, nom, STEP, EPOCH0_NS, end5, smooth_window=5)
    assert (l6 == 6).all() and (l5 == 5).all()
    np.testing.assert_array_equal(s5, r5)
    for i in (0, 100, 255):
        np.testing.assert_array_equal(s6[:, :, i], smooth_ric(r6[:, :, i].T, 5).T)
    assert not np.array_equal(s6, r6)


def _ragged(traj):
    """The same batch with every third trajectory cut to its first 150 states: series of two lengths."""
    t = copy.copy(traj)
    t.len = traj.len.copy()
    t.len[::3] = 150
    return t


def test_3_moments_are_reproducible_and_inside_the_summation_bound(leo, leo256):
    ctx = leo[4]
    traj, nom, _ = leo256
    rag = _ragged(traj)
    for batch, window in ((traj, 5), (rag, 0)):
        vals, length, _, mom = ctx.traj_ric_diff(batch, nom, STEP, capacity=181, smooth_window=window, moments=True)
        again = ctx.traj_ric_diff(batch, nom, STEP, capacity=181, smooth_window=window, moments=True)
        assert mom.shape == (181, 28)
        assert mom.tobytes() == again[3].tobytes() and vals.tobytes() == again[0].tobytes()      # identical bits on a repeated call
        plain, l0, _, none = ctx.traj_ric_diff(batch, nom, STEP, capacity=181, smooth_window=window)
        assert none is None and plain.tobytes() == vals.tobytes()                                # asking for the sums changes no value
        for k in range(181):
            have = np.nonzero(k < length)[0]
            assert np.isfinite(vals[:, k, have]).all() and np.isnan(vals[:, k, np.nonzero(k >= length)[0]]).all()
            assert_moments_within_the_summation_bound(mom[k], vals[:, k, have].T)                # (after smoothing)
    assert length.min() < 181 and length.max() == 181 and mom[:, 0].min() == 256 - 86 and mom[:, 0].max() == 256
    # the statistics they are made for
    count, mean, cov = nx.mc.ric_mean_cov(mom)
    np.testing.assert_allclose(mean[0], vals[:, 0, :].mean(axis=1), rtol=1e-11, atol=1e-14)
    np.testing.assert_allclose(cov[0], np.cov(vals[:, 0, :], ddof=1), rtol=1e-8)


def test_4_capacity_below_the_produced_count(leo, leo256):
    ctx = leo[4]
    lib = _abi.load_library()
    traj, nom, _ = leo256
    n, cap, guard = traj.n, 50, 1000
    raw, _, _, _ = ctx.traj_ric_diff(traj, nom, STEP, capacity=181, smooth_window=0)
    cin, cref = traj.as_c(), nom.as_c()
    for window in (0, 5):
        buf = np.full(6 * cap * n + guard, 12345.0)
        length = np.full(n + 8, -7, dtype=np.int32)
        epoch0 = np.full(n + 8, -7, dtype=np.int64)
        mom = np.full(cap * 28 + guard, 12345.0)
        q = _abi.RicQuery()
        q.step_ns, q.frame_of, q.transport, q.smooth_window = STEP, 1, 1, window
        rc = lib.nyx_hip_traj_ric_diff(ctx._h, C.byref(cin), n, C.byref(cref), 1, C.byref(q), cap, buf.ctypes.data_as(_abi.c_double_p),
                                       length.ctypes.data_as(_abi.c_int32_p), epoch0.ctypes.data_as(_abi.c_int64_p), mom.ctypes.data_as(_abi.c_double_p))
        assert rc == 0, _abi.last_error()
        assert (length[:n] == 181).all() and (length[n:] == -7).all()            # produced, not stored
        assert (epoch0[:n] == EPOCH0_NS).all() and (epoch0[n:] == -7).all()
        got = buf[: 6 * cap * n].reshape(6, cap, n)
        if window == 0:
            np.testing.assert_array_equal(got, raw[:, :cap])
        else:       # the filter works on the STORED samples
            for i in range(0, n, 5):
                np.testing.assert_array_equal(got[:, :, i], smooth_ric(raw[:, :cap, i].T, 5).T)
        assert (buf[6 * cap * n:] == 12345.0).all()                               # nothing beyond 6 * capacity * n
        assert (mom[cap * 28:] == 12345.0).all() and (mom[: cap * 28].reshape(cap, 28)[:, 0] == n).all()
        # epoch0_ns and moments are optional
        buf2, len2 = np.full(6 * cap * n, 12345.0), np.full(n, -7, dtype=np.int32)
        rc = lib.nyx_hip_traj_ric_diff(ctx._h, C.byref(cin), n, C.byref(cref), 1, C.byref(q), cap, buf2.ctypes.data_as(_abi.c_double_p),
                                       len2.ctypes.data_as(_abi.c_int32_p), None, None)
        assert rc == 0, _abi.last_error()
        np.testing.assert_array_equal(buf2, buf[: 6 * cap * n])
        np.testing.assert_array_equal(len2, length[:n])


def test_5_back_propagated_batch_short_reference_and_empty_overlap(leo, leo256):
    ctx = leo[4]
    dur = 5400 * S
    b = dispersed_leo_batch(65, seed=31, nominal=NOMINAL)
    _, st, back = ctx.propagate_with_traj(b, -dur, capacity=200)
    _, st1, nom_back = ctx.propagate_with_traj(_nominal_batch(), -dur, capacity=200)
    assert (st.status == 0).all() and (st1.status == 0).all() and back.epoch_ns[1, 0] < back.epoch_ns[0, 0]
    vals, length, epoch0, mom = ctx.traj_ric_diff(back, nom_back, STEP, capacity=96, smooth_window=0, moments=True)
    lo, count = expected_series(back, nom_back, STEP)
    np.testing.assert_array_equal(length, count)
    np.testing.assert_array_equal(epoch0, lo)
    assert (length == 91).all() and (epoch0 == EPOCH0_NS - dur).all()          # the series starts at the EARLIEST epoch
    rv, _ = every_states(ctx, back, STEP, 96)
    rr, _ = every_states(ctx, nom_back, STEP, 96)
    assert_within(vals[:, :91].transpose(1, 2, 0), ric_difference(rv[:91], rr[:91]), "back-propagated")
    assert np.isnan(vals[:, 91:]).all() and (mom[:91, 0] == 65).all() and (mom[91:] == 0).all()
    # the last sample is the start state of the propagation: the dispersion that was drawn
    assert_within(vals[:, 90].T, ric_difference(b.rv(), NOMINAL), "start states")
    # a reference shorter than the runs ends every series where IT ends
    traj, nom, _ = leo256
    _, st2, short = ctx.propagate_with_traj(_nominal_batch(), 3600 * S, capacity=200)
    assert (st2.status == 0).all()
    v_s, l_s, e_s, _ = ctx.traj_ric_diff(traj, short, STEP, smooth_window=0)
    full, _, _, _ = ctx.traj_ric_diff(traj, nom, STEP, capacity=181, smooth_window=0)
    assert v_s.shape == (6, 61, 256) and (l_s == 61).all() and (e_s == EPOCH0_NS).all()
    rv, _ = every_states(ctx, traj, STEP, 61)
    rr, rl = every_states(ctx, short, STEP, 61)
    assert (rl == 61).all()
    assert_within(v_s.transpose(1, 2, 0), ric_difference(rv, rr), "short nominal")
    # no overlap: a forward ensemble against a back-propagated nominal share ONE epoch; a window away from it shares none
    v1, l1, e1, m1 = ctx.traj_ric_diff(traj, nom_back, STEP, moments=True)
    assert v1.shape == (6, 1, 256) and (l1 == 1).all() and (e1 == EPOCH0_NS).all() and m1[0, 0] == 256
    v0, l0, e0, m0 = ctx.traj_ric_diff(traj, nom_back, STEP, EPOCH0_NS + STEP, EPOCH0_NS + 9 * STEP, capacity=4, moments=True)
    assert (l0 == 0).all() and (e0 == 0).all() and np.isnan(v0).all() and (m0 == 0).all()
    after = EPOCH0_NS + 4 * 3600 * S
    v0, l0, e0, m0 = ctx.traj_ric_diff(traj, nom, STEP, after, after + 10 * STEP, moments=True)
    assert v0.shape == (6, 1, 256) and (l0 == 0).all() and (e0 == 0).all() and np.isnan(v0).all() and (m0 == 0).all()
    # an empty reference, an empty run
    empty = copy.copy(nom)
    empty.len = np.zeros_like(nom.len)
    v0, l0, e0, _ = ctx.traj_ric_diff(traj, empty, STEP, capacity=3)
    assert (l0 == 0).all() and (e0 == 0).all() and np.isnan(v0).all()
    some = copy.copy(traj)
    some.len = traj.len.copy()
    some.len[[3, 200]] = 0
    v0, l0, e0, m0 = ctx.traj_ric_diff(some, nom, STEP, capacity=181, smooth_window=0, moments=True)
    assert l0[3] == 0 and l0[200] == 0 and np.isnan(v0[:, :, [3, 200]]).all() and (np.delete(l0, [3, 200]) == 181).all() and (m0[:, 0] == 254).all()
    np.testing.assert_array_equal(np.delete(v0, [3, 200], axis=2), np.delete(full, [3, 200], axis=2))


def test_6_the_series_ends_where_the_reference_cannot_be_interpolated(leo):
    """Two stored states of the REFERENCE 10 ns apart are the same f64 second: InterpMath for every window that holds them.
    The series of every run ends at the first such sample - either trajectory failing ends it, the reference zips two
    iterators that each stop at their first failure - and what later chunks could interpolate again is blanked."""
    ctx = leo[4]
    rng = np.random.default_rng(9)
    t = _abi.TrajBatch(3, 40)
    ref = _abi.TrajBatch(1, 40)
    for b in (t, ref):
        b.len[:] = 40
        for i in range(b.n):
            b.epoch_ns[:, i] = EPOCH0_NS + i * 13 + np.cumsum(rng.integers(5, 120, size=40)) * 10**9 + rng.integers(0, 10**9, size=40)
        b.state[:] = rng.standard_normal(b.state.shape) * 7000.0
    ref.epoch_ns[18, 0] = ref.epoch_ns[17, 0] + 10           # (the windows of the first samples, states 0 .. 12, do not hold it)
    t.epoch_ns[31, 2] = t.epoch_ns[30, 2] + 10               # run 2 has a pair of its own, later
    step = 10**9
    vals, length, epoch0, mom = ctx.traj_ric_diff(t, ref, step, capacity=4096, smooth_window=0, moments=True)
    lo, count = expected_series(t, ref, step)
    np.testing.assert_array_equal(epoch0, lo)
    for i in range(3):
        q = int(lo[i]) + step * np.arange(int(count[i]))
        a, sa = ctx.traj_at(t, q)
        b, sb = ctx.traj_at(ref, q)
        bad = np.nonzero(_abi.interp_failed(sa[:, i]) | _abi.interp_failed(sb[:, 0]))[0]
        ref_bad = np.nonzero(_abi.interp_failed(sb[:, 0]))[0]
        assert len(ref_bad) and 0 < bad[0] < count[i] and length[i] == bad[0]
        if i < 2:
            assert bad[0] == ref_bad[0] and not _abi.interp_failed(sa[:, i]).any()       # it is the reference that ends it
        m = int(length[i])
        assert_within(vals[:, :m, i].T, ric_difference(a[:m, i], b[:m, 0]), f"run {i}")
        assert np.isnan(vals[:, m:, i]).all()
        # ... although later samples can be interpolated again in both: blanked all the same
        late = np.nonzero(~_abi.interp_failed(sa[:, i]) & ~_abi.interp_failed(sb[:, 0]))[0]
        assert late[-1] > m + 16
    for k in range(int(length.max())):
        assert mom[k, 0] == (k < length).sum()
    assert (mom[int(length.max()):] == 0).all()


def test_7_device_pointers_on_a_stream_equal_the_host_flavour(leo, leo256):
    import torch
    ctx = leo[4]
    lib = _abi.load_library()
    dev = torch.device("cuda", 0)
    traj, _, pair = leo256
    n, cap, guard = traj.n, 100, 512
    start, stop = EPOCH0_NS + 500 * S, EPOCH0_NS + 9000 * S
    keep = []

    def on_device(t):
        epoch, state, tlen = torch.from_numpy(t.epoch_ns).to(dev), torch.from_numpy(t.state).to(dev), torch.from_numpy(t.len).to(dev)
        keep.extend([epoch, state, tlen])
        s = _abi.Traj()
        s.capacity = t.capacity
        s.epoch_ns = C.cast(epoch.data_ptr(), _abi.c_int64_p)
        for k, f in enumerate(["x_km", "y_km", "z_km", "vx_km_s", "vy_km_s", "vz_km_s"]):
            setattr(s, f, C.cast(state[k].data_ptr(), _abi.c_double_p))
        s.len = C.cast(tlen.data_ptr(), _abi.c_int32_p)
        return s

    for ref in (leo256[1], pair):
        host, host_len, host_e0, host_mom = ctx.traj_ric_diff(traj, ref, STEP, start, stop, capacity=cap, frame_of="run", smooth_window=5, moments=True)
        s, r = on_device(traj), on_device(ref)
        values = torch.full((6 * cap * n + guard,), 12345.0, dtype=torch.float64, device=dev)
        length = torch.full((n + 8,), -7, dtype=torch.int32, device=dev)
        epoch0 = torch.full((n + 8,), -7, dtype=torch.int64, device=dev)
        mom = torch.full((cap * 28 + guard,), 12345.0, dtype=torch.float64, device=dev)
        q = _abi.RicQuery()
        q.step_ns, q.has_window, q.start_ns, q.end_ns, q.frame_of, q.transport, q.smooth_window = STEP, 1, start, stop, 0, 1, 5
        stream = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(stream):
            rc = lib.nyx_hip_traj_ric_diff_device(ctx._h, C.byref(s), n, C.byref(r), ref.n, C.byref(q), cap, C.c_void_p(values.data_ptr()),
                                                  C.c_void_p(length.data_ptr()), C.c_void_p(epoch0.data_ptr()), C.c_void_p(mom.data_ptr()),
                                                  C.c_void_p(stream.cuda_stream))
        assert rc == 0, _abi.last_error()
        stream.synchronize()
        got, got_len, got_e0, got_mom = values.cpu().numpy(), length.cpu().numpy(), epoch0.cpu().numpy(), mom.cpu().numpy()
        np.testing.assert_array_equal(got_len[:n], host_len)
        np.testing.assert_array_equal(got_e0[:n], host_e0)
        assert (got_len[n:] == -7).all() and (got_e0[n:] == -7).all() and (host_len == 142).all() and (host_e0 == start).all()
        np.testing.assert_array_equal(got[: 6 * cap * n].reshape(6, cap, n), host)
        np.testing.assert_array_equal(got_mom[: cap * 28].reshape(cap, 28), host_mom)
        assert (got[6 * cap * n:] == 12345.0).all() and (got_mom[cap * 28:] == 12345.0).all()     # guard values: nothing beyond the buffers


def test_8_bad_arguments_launch_nothing(leo, leo256):
    ctx = leo[4]
    lib = _abi.load_library()
    traj, nom, pair = leo256
    ctx.traj_ric_diff(traj, nom, STEP, capacity=4)
    ms = ctx.last_kernel_ms()
    n = traj.n
    buf, length, epoch0, mom = np.full(6 * 4 * n, 12345.0), np.full(n, -7, dtype=np.int32), np.full(n, -7, dtype=np.int64), np.full(4 * 28, 12345.0)
    cin, cref = traj.as_c(), nom.as_c()

    def call(step=STEP, cap=4, n_=n, n_ref=1, frame_of=1, transport=1, window=5, values=buf, lens=length):
        q = _abi.RicQuery()
        q.step_ns, q.frame_of, q.transport, q.smooth_window = step, frame_of, transport, window
        return lib.nyx_hip_traj_ric_diff(ctx._h, C.byref(cin), n_, C.byref(cref), n_ref, C.byref(q), cap,
                                         None if values is None else values.ctypes.data_as(_abi.c_double_p),
                                         None if lens is None else lens.ctypes.data_as(_abi.c_int32_p), epoch0.ctypes.data_as(_abi.c_int64_p),
                                         mom.ctypes.data_as(_abi.c_double_p))

    for kw, why in [(dict(step=0), "step_ns"), (dict(step=-STEP), "step_ns"), (dict(cap=0), "capacity"), (dict(n_=-1, n_ref=-1), "negative n"),
                    (dict(n_ref=2), "n_ref = 2"), (dict(n_ref=0), "n_ref = 0"), (dict(frame_of=2), "frame_of"), (dict(frame_of=-1), "frame_of"),
                    (dict(transport=2), "transport"), (dict(window=4), "smooth_window"), (dict(window=11), "smooth_window"),
                    (dict(window=-3), "smooth_window"), (dict(values=None), "required"), (dict(lens=None), "required")]:
        assert call(**kw) == _abi.RC_BAD_ARG and why in _abi.last_error(), (kw, _abi.last_error())
    assert (buf == 12345.0).all() and (length == -7).all() and (epoch0 == -7).all() and (mom == 12345.0).all() and ctx.last_kernel_ms() == ms
    assert call() == 0 and (length == 181).all() and (epoch0 == EPOCH0_NS).all() and (mom.reshape(4, 28)[:, 0] == n).all()
    with pytest.raises(ValueError):
        ctx.traj_ric_diff(traj, nom, STEP, start_ns=EPOCH0_NS)
    with pytest.raises(ValueError):
        ctx.traj_ric_diff(traj, nom, STEP, frame_of="orbit")
    with pytest.raises(RuntimeError, match="smooth_window"):
        ctx.traj_ric_diff(traj, nom, STEP, capacity=4, smooth_window=6)
    with pytest.raises(ValueError):
        ctx.traj_ric_diff(traj, _two(pair), STEP)


def _two(batch):
    """The first two trajectories of a batch: neither one reference nor one per run."""
    t = _abi.TrajBatch(2, batch.capacity)
    t.len[:] = batch.len[:2]
    t.epoch_ns[:] = batch.epoch_ns[:, :2]
    t.state[:] = batch.state[:, :, :2]
    return t


def test_9_results_ric_dispersions_on_a_real_monte_carlo(leo):
    prop, almanac, central, _, ctx = leo
    template = nx.Spacecraft(EPOCH0_NS, leo_nominal(), central, dry_mass_kg=100.0, prop_mass_kg=10.0, srp_area_m2=1.0, cr=1.8)

    class Mc(nx.MonteCarlo):
        def generate_states(self, skip, num_runs, seed=None):
            out = super().generate_states(skip, num_runs, seed)
            out[4][1].dry_mass_kg = 0.0      # massless with a force model: that run errors (as tests/test_gpu_interface.py makes one fail)
            out[4][1].prop_mass_kg = 0.0
            return out

    mc = Mc(nx.MvnSpacecraft.from_sigmas(template, [1.0, 1.0, 1.0, 1e-3, 1e-3, 1e-3]), seed=5)
    res = mc.run_until_epoch(prop, almanac, EPOCH0_NS + 3600 * S, 12, capacity=256)
    assert isinstance(res.runs[4].result, nx.PropagationError) and len(res.ok_runs()) == 11
    _, st, nom = ctx.propagate_with_traj(nx.pack_spacecraft([template], False), 3600 * S, capacity=256)
    assert (st.status == 0).all()
    mc_ctx = res._traj_ctx
    assert hasattr(mc_ctx, "traj_ric_diff")

    class Compose:   # the evaluator of the definition: traj_every / traj_at only
        traj_at = staticmethod(mc_ctx.traj_at)
        traj_every = staticmethod(mc_ctx.traj_every)

    for kw in (dict(), dict(frame_of="run", transport=False, smooth_window=0), dict(start_ns=EPOCH0_NS + 400 * S, end_ns=EPOCH0_NS + 5000 * S, smooth_window=3)):
        rs = res.ric_dispersions(nom, STEP, **kw)
        want = dataclasses.replace(res, _traj_ctx=Compose).ric_dispersions(nom, STEP, **kw)
        k_n = 54 if "start_ns" in kw else 61
        assert isinstance(rs, nx.RicSeries) and rs.values.shape == want.values.shape == (6, k_n, 12)
        np.testing.assert_array_equal(rs.len, want.len)
        np.testing.assert_array_equal(rs.epoch0_ns, want.epoch0_ns)
        np.testing.assert_array_equal(rs.ok, want.ok)
        np.testing.assert_array_equal(rs.count, want.count)
        assert rs.len[4] == 0 and not rs.ok[4] and np.isnan(rs.values[:, :, 4]).all() and list(np.delete(rs.len, 4)) == [k_n] * 11
        assert (rs.count == 11).all()                                               # the failed run has no share in the statistics
        okc = np.nonzero(rs.ok)[0]
        assert_within(rs.values[:, :, okc].transpose(1, 2, 0), want.values[:, :, okc].transpose(1, 2, 0), f"Results.ric_dispersions {sorted(kw)}")
        for k in range(k_n):
            assert_moments_within_the_summation_bound(rs.moments[k], rs.values[:, k, okc].T)
            assert_moments_within_the_summation_bound(want.moments[k], want.values[:, k, okc].T)
        np.testing.assert_allclose(rs.mean, want.mean, rtol=1e-11, atol=1e-14)
        np.testing.assert_allclose(rs.cov, want.cov, rtol=1e-7, atol=1e-12 * np.abs(want.cov).max())
        np.testing.assert_allclose(rs.cov[0], np.cov(rs.values[:, 0, okc], ddof=1), rtol=1e-8, atol=1e-12 * np.abs(want.cov).max())
    # one pair through Traj.ric_diff: this trajectory minus the other, in the frame asked for
    run0 = res.runs[0].result.traj
    rs = res.ric_dispersions(nom, STEP)
    ep, d = run0.ric_diff(nx.Traj(mc_ctx, nom), STEP, frame_of="reference")
    assert list(ep) == [EPOCH0_NS + k * STEP for k in range(61)]
    np.testing.assert_array_equal(d, rs.values[:, :, 0])
    ep, own = run0.ric_diff(nx.Traj(mc_ctx, nom), STEP)                              # the reference's self.ric_difference(&other)
    np.testing.assert_array_equal(own, res.ric_dispersions(nom, STEP, frame_of="run").values[:, :, 0])
