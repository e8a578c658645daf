"""Fused device reports (report_kernel.hip, include/nyx_hip_reports.h) on the MI355X.

The interpolated state a parameter is evaluated from is the one `traj_every` / `traj_at` return (same device code), so
X .. VZ must come back BIT-IDENTICAL; the other parameters are compared with `nyx_amd.params.state_value` (numpy) applied
to those states, so the only difference is the device's libm (sqrt, pow, acos, atan2, fmod) and the rounding of a few
operations.  Small on purpose: a few hundred trajectories, hours, 8x8 gravity.

TOLERANCES (test 2).  Measured on the MI355X (256 dispersed LEO trajectories, e = 0.05, i = 68.5 deg, 3 h, one sample
per 60 s = 46 336 samples per parameter): the largest |device - state_value|, relative to |value| for the non-angles,
in degrees (difference wrapped to [-180, 180)) for the angles.  The bound is the measured figure x 8 rounded up to one
significant digit - the run is deterministic, the margin covers a compiler or libm change of a few ulp - and never above
the ceilings 1e-9 (relative) / 1e-6 deg.  A measured 0 stays 0: those are exact.

    parameter         measured    unit  bound
    X                 0           rel   0
    Y                 0           rel   0
    Z                 0           rel   0
    VX                0           rel   0
    VY                0           rel   0
    VZ                0           rel   0
    Rmag              0           rel   0
    Vmag              0           rel   0
    Hmag              0           rel   0
    Energy            0           rel   0
    SemiMajorAxis     0           rel   0
    Eccentricity      0           rel   0
    Inclination       0           deg   0
    RAAN              0           deg   0
    AoP               2.842e-14   deg   3e-13
    TrueAnomaly       5.684e-14   deg   5e-13
    Period            3.107e-16   rel   3e-15
    ApoapsisRadius    0           rel   0
    PeriapsisRadius   0           rel   0

The zeros are no accident: sqrt, division and the products are IEEE operations done in numpy's order; acos and the atan2 of
RAAN agreed with numpy's to the last bit on every sample.  The three non-zero rows are one or two ulp of atan2 / pow.
"""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import nyx_amd as nx
from nyx_amd import _abi
from nyx_amd.params import StateParameter as P, state_value
from nyx_amd import ephem
from scenarios import EARTH_RADIUS_KM, EPOCH0_NS, dispersed_leo_batch, keplerian_to_cartesian, leo_full_setup, leo_nominal

pytestmark = pytest.mark.gpu

S = nx.NS_PER_S
STEP = 60 * S
CART = [P.X, P.Y, P.Z, P.VX, P.VY, P.VZ]
ORBIT = [p for p in P if p.name in _abi.STATE_PARAM]
ANGLES = {P.Inclination, P.RAAN, P.AoP, P.TrueAnomaly}
CEILING_REL, CEILING_DEG = 1e-9, 1e-6
# parameter -> bound (relative, or degrees for the angles): see the table above
TOL = {
    P.X: 0.0,
    P.Y: 0.0,
    P.Z: 0.0,
    P.VX: 0.0,
    P.VY: 0.0,
    P.VZ: 0.0,
    P.Rmag: 0.0,
    P.Vmag: 0.0,
    P.Hmag: 0.0,
    P.Energy: 0.0,
    P.SemiMajorAxis: 0.0,
    P.Eccentricity: 0.0,
    P.Inclination: 0.0,
    P.RAAN: 0.0,
    P.AoP: 3e-13,
    P.TrueAnomaly: 5e-13,
    P.Period: 3e-15,
    P.ApoapsisRadius: 0.0,
    P.PeriapsisRadius: 0.0,
}


def deviation(p, got, want):
    """Largest difference of one parameter over the samples: relative for the non-angles, wrapped degrees for the angles."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and np.isfinite(want).all() and np.isfinite(got).all(), p.name
    if p in ANGLES:
        return float(np.abs((got - want + 180.0) % 360.0 - 180.0).max()) if got.size else 0.0
    return float((np.abs(got - want) / np.abs(want)).max()) if got.size else 0.0


def assert_within(p, got, want):
    d = deviation(p, got, want)
    print(f"deviation {p.name:16s} {d:.3e}  (bound {TOL[p]:.0e})")
    assert TOL[p] <= (CEILING_DEG if p in ANGLES else CEILING_REL)
    assert d <= TOL[p], f"{p.name}: {d:.3e} > {TOL[p]:.0e}"


@pytest.fixture(scope="module")
def leo():
    prop, almanac, central = leo_full_setup(degree=8)
    compiled = prop.compile(almanac, central)
    ctx = nx.GpuContext(compiled)
    yield prop, almanac, central, compiled, ctx
    ctx.close()


@pytest.fixture(scope="module")
def leo256(leo):
    ctx = leo[4]
    # e = 0.05 over a 300 km perigee: the osculating eccentricity stays above 0.01 under J2 (the 0.015 of leo_nominal dips to 0.005)
    nominal = keplerian_to_cartesian((EARTH_RADIUS_KM + 300.0) / 0.95, 0.05, 68.5, 65.2, 75.0, 0.0, ephem.MU_EARTH)
    b = dispersed_leo_batch(256, seed=11, nominal=nominal)
    out, st, traj = ctx.propagate_with_traj(b, 3 * 3600 * S, capacity=400)
    assert (st.status == 0).all()
    return traj


def every_states(ctx, traj, step, cap):
    """(states[K, n, 6], len[n]) of traj_every."""
    ev = ctx.traj_every(traj, step, cap)
    return np.ascontiguousarray(ev.state.transpose(1, 2, 0)), ev.len, ev


def check_cartesian(ctx, traj, step, cap):
    ev = ctx.traj_every(traj, step, cap)
    vals, length = ctx.traj_values(traj, CART, step, capacity=cap)
    assert vals.shape == (6, cap, traj.n) and length.dtype == np.int32
    np.testing.assert_array_equal(length, ev.len)
    for i in range(traj.n):
        m = min(int(length[i]), cap)
        np.testing.assert_array_equal(vals[:, :m, i], ev.state[:, :m, i])      # bit for bit
        assert np.isnan(vals[:, m:, i]).all()                                  # the kernel blanks what it did not produce
    return vals, length


@pytest.mark.parametrize("n", [1, 65, 128])
def test_1_cartesian_values_are_the_traj_every_states_bit_for_bit(leo, n):
    ctx = leo[4]
    b = dispersed_leo_batch(n, seed=20 + n)
    dur = 2 * 3600 * S
    _, st, traj = ctx.propagate_with_traj(b, dur, capacity=300)
    assert (st.status == 0).all()
    vals, length = check_cartesian(ctx, traj, STEP, 128)
    assert (length == 121).all()
    np.testing.assert_array_equal(vals[:, 0, :], b.rv().T)
    # capacity=None: sized from the batch's epochs
    v2, l2 = ctx.traj_values(traj, CART, STEP)
    assert v2.shape == (6, 121, n)
    np.testing.assert_array_equal(v2, vals[:, :121])
    np.testing.assert_array_equal(l2, length)
    # a step that does not divide the span, ragged last chunk
    check_cartesian(ctx, traj, 47 * S + 13, 160)


def test_2_all_parameters_against_state_value(leo, leo256):
    ctx, central = leo[4], leo[2]
    rv, ln, _ = every_states(ctx, leo256, STEP, 181)
    assert (ln == 181).all()
    vals, length = ctx.traj_values(leo256, ORBIT, STEP, capacity=181)       # 19 parameters: three launches
    np.testing.assert_array_equal(length, ln)
    ecc = state_value(P.Eccentricity, rv, central.mu_km3_s2)
    inc = state_value(P.Inclination, rv, central.mu_km3_s2)
    assert ecc.min() >= 0.01 and 10.0 < inc.min() and inc.max() < 170.0     # where the numpy definition is well conditioned
    assert set(TOL) == set(ORBIT)
    failures = []
    for j, p in enumerate(ORBIT):
        want = state_value(p, rv, central.mu_km3_s2)
        try:
            assert_within(p, vals[j], want)
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, "\n".join(failures)
    for j, p in enumerate(ORBIT[:6]):
        np.testing.assert_array_equal(vals[j], rv[..., j])


def _mc(ctx_prop, runs=70, end=EPOCH0_NS + 5400 * S, fail=None):
    prop, almanac, central = ctx_prop
    template = nx.Spacecraft(EPOCH0_NS, leo_nominal(), central, dry_mass_kg=100.0, prop_mass_kg=10.0, srp_area_m2=1.0, cr=1.8)

    class Mc(nx.MonteCarlo):
        def generate_states(self, skip, num_runs, seed=None):
            out = super().generate_states(skip, num_runs, seed)
            if fail is not None:   # massless with a force model: that run errors (as tests/test_gpu_interface.py makes one fail)
                out[fail][1].dry_mass_kg = 0.0
                out[fail][1].prop_mass_kg = 0.0
            return out

    mc = Mc(nx.MvnSpacecraft.from_sigmas(template, [1.0, 1.0, 1.0, 1e-3, 1e-3, 1e-3]), seed=5)
    return mc.run_until_epoch(prop, almanac, end, runs, capacity=256)


def test_3_windows_against_the_per_run_path(leo):
    res = _mc(leo[:3])
    end = EPOCH0_NS + 5400 * S
    params = [P.X, P.VY, P.Rmag, P.SemiMajorAxis, P.TrueAnomaly]
    windows = [(EPOCH0_NS - 1000 * S, EPOCH0_NS + 2000 * S),      # starts before the runs: clamped to their first epoch
               (EPOCH0_NS + 777 * S, end + 500 * S),              # starts inside, ends after: clamped to their last epoch
               (EPOCH0_NS + 1000 * S + 1, EPOCH0_NS + 1000 * S + 1),   # one interpolated sample
               (end + S, end + 100 * S)]                          # starts after the runs: nothing
    for start, stop in windows:
        vs = res.values_of(params, STEP, start, stop)
        lo, hi = max(start, EPOCH0_NS), min(stop, end)
        want_len = (hi - lo) // STEP + 1 if hi >= lo else 0
        assert (vs.len == want_len).all() and vs.values.shape == (len(params), want_len, 70)
        for p in params:
            listed = np.array(res.every_value_of_between(p, STEP, start, stop))       # one traj_at launch per run
            assert listed.shape == (70 * want_len,)
            got = vs.values[vs.params.index(p)].T.reshape(-1)                         # run after run
            if p in CART:
                np.testing.assert_array_equal(got, listed)
            else:
                assert_within(p, got, listed)
        if want_len:
            assert (vs.epoch0_ns == lo).all()


def test_4_capacity_below_the_produced_count(leo, leo256):
    ctx = leo[4]
    lib = _abi.load_library()
    n, cap, guard = leo256.n, 50, 1000
    full, full_len = ctx.traj_values(leo256, [P.Y, P.Eccentricity], STEP, capacity=181)
    buf = np.full(2 * cap * n + guard, 12345.0)
    length = np.full(n + 8, -7, dtype=np.int32)
    q = _abi.ValuesQuery()
    q.n_params, q.step_ns = 2, STEP
    q.param[0], q.param[1] = _abi.STATE_PARAM["Y"], _abi.STATE_PARAM["Eccentricity"]
    cin = leo256.as_c()
    rc = lib.nyx_hip_traj_values(ctx._h, C.byref(cin), n, C.byref(q), cap, buf.ctypes.data_as(_abi.c_double_p), length.ctypes.data_as(_abi.c_int32_p))
    assert rc == 0, _abi.last_error()
    assert (length[:n] == 181).all() and (length[n:] == -7).all()            # produced, not stored
    np.testing.assert_array_equal(buf[: 2 * cap * n].reshape(2, cap, n), full[:, :cap])
    assert (buf[2 * cap * n:] == 12345.0).all()                               # nothing beyond n_params * capacity * n


def test_5_eight_in_one_launch_equal_eight_launches_and_the_split_of_nine(leo, leo256):
    ctx = leo[4]
    eight = [P.SemiMajorAxis, P.Eccentricity, P.Inclination, P.RAAN, P.AoP, P.TrueAnomaly, P.Rmag, P.Period]
    together, ln = ctx.traj_values(leo256, eight, STEP, capacity=181)
    for j, p in enumerate(eight):
        alone, l1 = ctx.traj_values(leo256, [p], STEP, capacity=181)
        np.testing.assert_array_equal(alone[0], together[j], err_msg=p.name)
        np.testing.assert_array_equal(l1, ln)
    nine = eight + [P.Energy]
    split, l9 = ctx.traj_values(leo256, nine, STEP, capacity=181)
    assert split.shape == (9, 181, leo256.n)
    np.testing.assert_array_equal(split[:8], together)
    np.testing.assert_array_equal(split[8], ctx.traj_values(leo256, [P.Energy], STEP, capacity=181)[0][0])
    np.testing.assert_array_equal(l9, ln)
    with pytest.raises(nx.StateError):
        ctx.traj_values(leo256, [P.X, P.Cr], STEP)


def test_6_back_propagated_batch(leo):
    ctx = leo[4]
    b = dispersed_leo_batch(65, seed=31)
    dur = 5400 * S
    out, st, back = ctx.propagate_with_traj(b, -dur, capacity=200)
    assert (st.status == 0).all() and back.epoch_ns[1, 0] < back.epoch_ns[0, 0]
    vals, length = check_cartesian(ctx, back, STEP, 96)
    assert (length == 91).all()
    np.testing.assert_array_equal(vals[:, 0, :], out.rv().T)          # the series starts at the EARLIEST epoch: the end state
    np.testing.assert_array_equal(vals[:, 90, :], b.rv().T)
    # a window on it, against traj_at at the same epochs
    start = EPOCH0_NS - 3000 * S + 5
    wv, wl = ctx.traj_values(back, CART, STEP, start, EPOCH0_NS + 10 * S)
    assert (wl == 50).all() and wv.shape == (6, 50, 65)
    at, status = ctx.traj_at(back, start + STEP * np.arange(50))
    assert not _abi.interp_failed(status).any()
    np.testing.assert_array_equal(wv, at.transpose(2, 0, 1))


def test_7_device_pointers_on_a_stream_equal_the_host_flavour(leo, leo256):
    import torch
    ctx = leo[4]
    lib = _abi.load_library()
    dev = torch.device("cuda", 0)
    t = leo256
    n, cap, guard = t.n, 100, 512
    params = [P.Z, P.SemiMajorAxis, P.AoP]
    host, host_len = ctx.traj_values(t, params, STEP, EPOCH0_NS + 500 * S, EPOCH0_NS + 9000 * S, capacity=cap)
    epoch = torch.from_numpy(t.epoch_ns).to(dev)
    state = torch.from_numpy(t.state).to(dev)
    tlen = torch.from_numpy(t.len).to(dev)
    s = _abi.Traj()
    s.capacity = t.capacity
    s.epoch_ns = C.cast(epoch.data_ptr(), _abi.c_int64_p)
    for k, f in enumerate(["x_km", "y_km", "z_km", "vx_km_s", "vy_km_s", "vz_km_s"]):
        setattr(s, f, C.cast(state[k].data_ptr(), _abi.c_double_p))
    s.len = C.cast(tlen.data_ptr(), _abi.c_int32_p)
    values = torch.full((3 * cap * n + guard,), 12345.0, dtype=torch.float64, device=dev)
    length = torch.full((n + 8,), -7, dtype=torch.int32, device=dev)
    q = _abi.ValuesQuery()
    q.n_params, q.has_window, q.step_ns, q.start_ns, q.end_ns = 3, 1, STEP, EPOCH0_NS + 500 * S, EPOCH0_NS + 9000 * S
    for k, p in enumerate(params):
        q.param[k] = _abi.STATE_PARAM[p.name]
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        rc = lib.nyx_hip_traj_values_device(ctx._h, C.byref(s), n, C.byref(q), cap, C.c_void_p(values.data_ptr()), C.c_void_p(length.data_ptr()),
                                            C.c_void_p(stream.cuda_stream))
    assert rc == 0, _abi.last_error()
    stream.synchronize()
    got, got_len = values.cpu().numpy(), length.cpu().numpy()
    np.testing.assert_array_equal(got_len[:n], host_len)
    assert (got_len[n:] == -7).all() and (host_len == 142).all()               # (9000 - 500) / 60 + 1 produced, 100 stored
    np.testing.assert_array_equal(got[: 3 * cap * n].reshape(3, cap, n), host)
    assert (got[3 * cap * n:] == 12345.0).all()                                 # guard values: nothing beyond the buffer


def test_8_bad_arguments_launch_nothing(leo, leo256):
    ctx = leo[4]
    lib = _abi.load_library()
    ctx.traj_values(leo256, [P.X], STEP, capacity=4)
    ms = ctx.last_kernel_ms()
    n = leo256.n
    buf, length = np.full(8 * 4 * n, 12345.0), np.full(n, -7, dtype=np.int32)
    cin = leo256.as_c()

    def call(n_params=1, param=0, step=STEP, cap=4, values=buf, lens=length):
        q = _abi.ValuesQuery()
        q.n_params, q.step_ns = n_params, step
        for k in range(8):
            q.param[k] = param
        return lib.nyx_hip_traj_values(ctx._h, C.byref(cin), n, C.byref(q), cap, None if values is None else values.ctypes.data_as(_abi.c_double_p),
                                       None if lens is None else lens.ctypes.data_as(_abi.c_int32_p))

    for kw, why in [(dict(n_params=0), "n_params"), (dict(n_params=9), "n_params"), (dict(param=19), "not a nyx_hip_state_param"),
                    (dict(step=0), "step_ns"), (dict(step=-STEP), "step_ns"), (dict(cap=0), "capacity"), (dict(values=None), "required"),
                    (dict(lens=None), "required")]:
        assert call(**kw) == _abi.RC_BAD_ARG and why in _abi.last_error(), (kw, _abi.last_error())
    assert (buf == 12345.0).all() and (length == -7).all() and ctx.last_kernel_ms() == ms
    assert call() == 0 and (length == 181).all()


def test_9_results_values_of_on_a_real_monte_carlo(leo):
    res = _mc(leo[:3], runs=12, end=EPOCH0_NS + 3600 * S, fail=4)
    assert isinstance(res.runs[4].result, nx.PropagationError) and len(res.ok_runs()) == 11
    params = ORBIT + [P.Cr, P.TotalMass]
    vs = res.values_of(params, STEP, value_if_run_failed=-1.0)
    ctx = res._traj_ctx
    assert hasattr(ctx, "traj_values")

    class Compose:   # the evaluator of the definition: traj_every / traj_at only
        traj_at = staticmethod(ctx.traj_at)
        traj_every = staticmethod(ctx.traj_every)

    want = dataclasses.replace(res, _traj_ctx=Compose).values_of(params, STEP, value_if_run_failed=-1.0)
    assert vs.values.shape == want.values.shape == (len(params), 61, 12)
    np.testing.assert_array_equal(vs.len, want.len)
    np.testing.assert_array_equal(vs.epoch0_ns, want.epoch0_ns)
    np.testing.assert_array_equal(vs.ok, want.ok)
    assert vs.len[4] == 0 and (vs.values[:, :, 4] == -1.0).all() and list(np.delete(vs.len, 4)) == [61] * 11
    okc = np.nonzero(vs.ok)[0]
    for j, p in enumerate(params):
        if p in TOL and p not in CART:
            assert_within(p, vs.values[j][:, okc], want.values[j][:, okc])
        else:
            np.testing.assert_array_equal(vs.values[j], want.values[j], err_msg=p.name)
    assert vs.flat(P.X, -1.0) == res.every_value_of(P.X, STEP, value_if_run_failed=-1.0)
    # one trajectory through Traj.values_every
    ep, one = res.runs[0].result.traj.values_every([P.X, P.Rmag], STEP)
    assert list(ep) == [EPOCH0_NS + k * STEP for k in range(61)]
    np.testing.assert_array_equal(one[0], vs.values[0, :, 0])
    np.testing.assert_array_equal(one[1], vs.values[params.index(P.Rmag), :, 0])


def test_the_series_ends_at_the_first_sample_that_cannot_be_interpolated(leo):
    """Two stored states 10 ns apart are the same f64 second: InterpMath for every window that holds them.  The series
    of that trajectory ends there (traj_it.rs:39-61), as nyx_hip_traj_every reports, and what later chunks could
    interpolate again is blanked."""
    ctx = leo[4]
    rng = np.random.default_rng(9)
    t = _abi.TrajBatch(2, 20)
    t.len[:] = 20
    for i in range(2):
        t.epoch_ns[:, i] = EPOCH0_NS + i * 13 + np.cumsum(rng.integers(5, 120, size=20)) * 10**9 + rng.integers(0, 10**9, size=20)
    t.state[:] = rng.standard_normal(t.state.shape) * 7000.0
    t.epoch_ns[8, 1] = t.epoch_ns[7, 1] + 10
    ev = ctx.traj_every(t, 10**9, 4096)
    vals, length = ctx.traj_values(t, [P.X, P.Vmag], 10**9, capacity=4096)
    np.testing.assert_array_equal(length, ev.len)
    assert 0 < length[1] < length[0]             # trajectory 1 ends early: its first windows hold the coincident pair
    for i in range(2):
        m = int(length[i])
        np.testing.assert_array_equal(vals[0, :m, i], ev.state[0, :m, i])
        assert np.isfinite(vals[:, :m, i]).all() and np.isnan(vals[:, m:, i]).all()
    # ... although samples of LATER chunks can be interpolated again (their windows no longer hold the pair): blanked all the same
    first1 = int(t.epoch_ns[0, 1])
    k_late = int((t.epoch_ns[17, 1] - first1) // 10**9) + 1
    at, status = ctx.traj_at(t, [first1 + k_late * 10**9])
    assert status[0, 1] == _abi.INTERP_OK and np.isfinite(at[0, 1]).all() and k_late > 16 + length[1]
    assert np.isnan(vals[:, k_late, 1]).all()
