"""The encounter report on the MI355X (frame_kernel.hip, include/nyx_hip_frame.h).

The inertial state a value is evaluated from is the one `traj_every` / `traj_at` return (same device code), and the ephemerides, the
translation and the parameters are the code tests/test_frame_host_cxx.py runs on the CPU against the host definition: the values are
compared with `nyx_amd.frames.frame_value` applied to those states at their epochs.  Small on purpose: at most 70 trajectories, one
orbit.

THE ENSEMBLE is the fixture of tests/test_gpu_eclipse.py: `leo_full_setup(degree=8)`, `dispersed_leo_batch(70, seed=11)`, 5400 s,
capacity 256 - one full wave plus one with 6 live lanes.  Seen from the Moon (a chain of two segments) and from Jupiter (three) every
run is on a hyperbola - the fixtures assert it on the host definition -, seen from the Earth itself (the empty chain: the identity)
none is, and seen from the Sun (three) a run is on one for a part of every revolution only: the NaN-and-continue rule with and without
a translation, sample by sample.

TOLERANCES, from the number formats and not from a run.  Twenty of the twenty-five parameters are formed with + - * / sqrt and fabs
only, each a correctly rounded IEEE operation on both sides, in one order (csrc/frame_dev.h restates nyx_amd/frames.py operation for
operation, compiled with -ffp-contract=off): their bound is ZERO, as tests/test_gpu_reports.py and tests/test_gpu_eclipse.py find for
such values.  The angles (Inclination, RAAN, AoP, TrueAnomaly, BAngle) pass through acos / atan2: the device's (OpenCL bounds: 4 and
6 ulp) against glibc's or numpy's (1 .. 4 ulp), at most 10 ulp of a result of at most pi radians = 4.4e-15 rad = 2.6e-13 deg, plus the
scaling to degrees and the wrap on both sides, each an ulp of at most 360 = 5.7e-14 deg: bound 1e-12 deg (difference wrapped to
[-180, 180)).  Period = 2 pi sqrt(pow(sma, 3) / mu): pow within 16 ulp (OpenCL) against numpy's 1, halved by the square root, plus
the division, the root and the product on both sides: (17 / 2 + 3) eps = 2.6e-15, bound 4e-15 relative.  NaN must stand where the
definition has NaN, and nowhere else."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import nyx_amd as nx
from nyx_amd import _abi, eclipse, frames
from nyx_amd.frames import FrameParameter as F
from scenarios import EPOCH0_NS, dispersed_leo_batch, leo_full_setup, leo_nominal

pytestmark = pytest.mark.gpu

S = nx.NS_PER_S
STEP = 60 * S
DUR = 5400 * S
COUNT = 91
TILE = 8           # FRM_TILE of csrc/frame_kernel.hip
ALL = list(F)      # twenty-five: four launches through the Python split
ANGLES = (F.Inclination, F.RAAN, F.AoP, F.TrueAnomaly, F.BAngle)
TOL = {**{p: 0.0 for p in F}, **{p: 1e-12 for p in ANGLES}, F.Period: 4e-15}
BODIES = (nx.SUN, nx.MOON, nx.JUPITER_BARYCENTER)


def assert_all_within(params, got, want, label=""):
    """got / want [P, ...]: NaN where the definition has NaN, every parameter inside its bound elsewhere."""
    failures = []
    for j, p in enumerate(params):
        g, w = np.asarray(got[j]), np.asarray(want[j])
        assert g.shape == w.shape
        np.testing.assert_array_equal(np.isnan(g), np.isnan(w), err_msg=f"{p.name}{label}: NaN pattern")
        held = ~np.isnan(w)
        assert np.isfinite(g[held]).all() and np.isfinite(w[held]).all(), p.name
        if not held.any():
            d = 0.0
        elif p in ANGLES:
            d = float(np.abs((g[held] - w[held] + 180.0) % 360.0 - 180.0).max())
        elif p is F.Period:
            d = float((np.abs(g[held] - w[held]) / np.abs(w[held])).max())
        else:
            d = float(np.abs(g[held] - w[held]).max())
        print(f"deviation{label} {p.name:16s} {d:.3e}  (bound {TOL[p]:.0e}, {int(held.sum())} values)")
        if not d <= TOL[p]:
            failures.append(f"{p.name}{label}: {d:.3e} > {TOL[p]:.0e}")
    assert not failures, "\n".join(failures)


def host_values(world, params, rv, epochs, target):
    """[P, ...] of the host definition."""
    return np.stack([frames.frame_value(p, rv, epochs, target, world["almanac"], world["central"]) for p in params])


@pytest.fixture(scope="module")
def world():
    prop, almanac, central = leo_full_setup(degree=8)      # (every segment of the almanac is the context's: Jupiter's too)
    compiled = prop.compile(almanac, central)
    ctx = nx.GpuContext(compiled)
    targets = {naif: almanac.frame_info(naif) for naif in BODIES}
    yield dict(prop=prop, almanac=almanac, central=central, compiled=compiled, ctx=ctx, moon=targets[nx.MOON], sun=targets[nx.SUN],
               jupiter=targets[nx.JUPITER_BARYCENTER])
    ctx.close()


@pytest.fixture(scope="module")
def leo70(world):
    """One orbit of 70 dispersed trajectories with dense output, its traj_every states, the host definition about the Moon on those
    states and the device's twenty-five parameters at capacity 91: computed once, shared, never written to."""
    ctx = world["ctx"]
    _, st, traj = ctx.propagate_with_traj(dispersed_leo_batch(70, seed=11), DUR, capacity=256)
    assert (st.status == 0).all()
    ev = ctx.traj_every(traj, STEP, COUNT)
    assert (ev.len == COUNT).all()
    rv = np.ascontiguousarray(ev.state.transpose(1, 2, 0))             # [K, n, 6]
    want = host_values(world, ALL, rv, ev.epoch_ns, world["moon"])      # [25, K, n]
    assert [len(eclipse.body_chain(world[k].naif_id, world["almanac"], world["central"])) for k in ("moon", "sun", "jupiter")] == [2, 3, 3]
    assert (want[F.Eccentricity] > 1.0).all() and np.isnan(want[F.Period]).all()          # every sample on a hyperbola about the Moon
    assert np.isfinite(np.delete(want, int(F.Period), axis=0)).all()
    got, length = ctx.traj_frame_values(traj, world["moon"], ALL, STEP, capacity=COUNT)
    for a in (ev.state, ev.epoch_ns, rv, want, got, length):
        a.setflags(write=False)
    return traj, ev, rv, want, got, length


def head(traj, n):
    """The first n trajectories of a batch as a batch of their own."""
    t = _abi.TrajBatch(n, traj.capacity)
    t.epoch_ns[:], t.state[:], t.len[:] = traj.epoch_ns[:, :n], traj.state[:, :, :n], traj.len[:n]
    return t


def frame_query(world, target, params, step=STEP, start=None, stop=None):
    """The query GpuContext.traj_frame_values builds, for the raw entries."""
    q = _abi.FrameQuery()
    q.n_params, q.step_ns, q.mu_km3_s2 = len(params), step, float(target.mu_km3_s2)
    for k, p in enumerate(params):
        q.param[k] = int(p)
    if start is not None:
        q.has_window, q.start_ns, q.end_ns = 1, start, stop
    chain = eclipse.body_chain(target.naif_id, world["almanac"], world["central"])
    q.n_chain = len(chain)
    for k, (seg, sign) in enumerate(chain):
        q.chain_segment[k], q.chain_sign[k] = seg, sign
    return q


def test_1_full_orbit_all_parameters_about_the_moon(world, leo70):
    traj, rv, want, got, length = leo70[0], leo70[2], leo70[3], leo70[4], leo70[5]
    assert set(TOL) == set(F) and len(ALL) == 25
    assert got.shape == (25, COUNT, 70) and length.dtype == np.int32 and (length == COUNT).all()
    assert_all_within(ALL, got, want, label=" moon")
    # the figures hang together on the device's own values
    np.testing.assert_array_equal(got[F.BMagnitude], np.sqrt(got[F.BdotT] * got[F.BdotT] + got[F.BdotR] * got[F.BdotR]))
    np.testing.assert_array_equal(got[F.VInfinity], np.sqrt(got[F.C3]))
    np.testing.assert_array_equal(got[F.PeriapsisRadius], got[F.SemiMajorAxis] * (1.0 - got[F.Eccentricity]))
    assert ((got[F.BAngle] > -180.0) & (got[F.BAngle] <= 180.0)).all() and (got[F.Rmag] > 3.4e5).all() and (got[F.Rmag] < 4.2e5).all()
    with pytest.raises(TypeError):
        world["ctx"].traj_frame_values(traj, world["moon"], [F.Rmag, nx.AerParameter.Range], STEP)
    with pytest.raises(KeyError, match="planetary data"):
        world["ctx"].traj_frame_values(traj, nx.Frame(499, 42828.0), [F.Rmag], STEP)


def test_2_the_other_centres(world, leo70):
    """Jupiter: a chain of three, hyperbolic.  The Sun: a chain of three, hyperbolic for a part of the revolution only - NaN B-plane values there and the series goes on.
    The Earth itself: the empty chain, the values of nyx_hip_traj_values bit for bit."""
    ctx = world["ctx"]
    traj, ev, rv = leo70[0], leo70[1], leo70[2]
    params = [F.X, F.VZ, F.Rmag, F.Eccentricity, F.C3, F.BdotT, F.BdotR, F.VInfinity]
    for name, hyperbolic in (("jupiter", True), ("sun", False)):
        want = host_values(world, params, rv, ev.epoch_ns, world[name])
        bound_part = want[3] <= 1.0
        print(f"{name}: {int(bound_part.sum())} of {bound_part.size} samples are not hyperbolic")
        assert not bound_part.any() if hyperbolic else bound_part.any()
        assert (np.isnan(want[5:]) == bound_part[None]).all() and np.isfinite(want[:5]).all()
        got, length = ctx.traj_frame_values(traj, world[name], params, STEP)              # capacity=None: sized from the batch's epochs
        assert got.shape == (8, COUNT, 70) and (length == COUNT).all()                     # the series continues
        assert_all_within(params, got, want, label=f" {name}")
    orbit = [F.X, F.Y, F.Z, F.VX, F.VY, F.VZ, F.Rmag, F.SemiMajorAxis]
    got, length = ctx.traj_frame_values(traj, world["central"], orbit + [F.BdotT, F.BAngle, F.TrueAnomaly], STEP)
    same, l2 = ctx.traj_values(traj, [nx.StateParameter[p.name] for p in orbit] + [nx.StateParameter.TrueAnomaly], STEP)
    assert (length == COUNT).all() and (l2 == COUNT).all()
    np.testing.assert_array_equal(got[:8], same[:8])
    np.testing.assert_array_equal(got[10], same[8])
    np.testing.assert_array_equal(got[:6], ev.state[:, :COUNT])                            # the identity: the interpolated states themselves
    own = [F.BdotT, F.BAngle, F.TrueAnomaly]
    want = host_values(world, own + [F.Eccentricity], rv, ev.epoch_ns, world["central"])
    # NaN wherever the ellipse is - nearly everywhere: two dozen of the 6370 interpolated states, in the last two samples before the end of
    # a trajectory, come back from `traj_every` with a velocity of tens to hundreds of km/s, and the definition calls those hyperbolic too
    assert (np.isnan(want[:2]) == (want[3] <= 1.0)[None]).all() and (want[3] <= 1.0).mean() > 0.9
    assert_all_within(own, got[8:], want[:3], label=" earth")


def test_3_a_window_resolved_across_tile_seams(world, leo70):
    ctx = world["ctx"]
    traj = leo70[0]
    start, stop = EPOCH0_NS + 1140 * S, EPOCH0_NS + 1320 * S
    q = start + S * np.arange(181, dtype=np.int64)
    states, status = ctx.traj_at(traj, q)                                       # [181, 70, 6]
    assert not _abi.interp_failed(status).any()
    epochs = np.broadcast_to(q[:, None], states.shape[:2])
    params = [F.Rmag, F.PeriapsisRadius, F.C3, F.BdotT, F.BdotR, F.BAngle, F.Inclination, F.VY]
    want = host_values(world, params, states, epochs, world["moon"])
    got, length = ctx.traj_frame_values(traj, world["moon"], params, S, start, stop)
    assert got.shape == (8, 181, 70) and (length == 181).all()                 # 181 = 22 tiles of 8 + 5
    assert_all_within(params, got, want, label=" window")


@pytest.mark.parametrize("n", [1, 64, 65])
def test_4_seams_and_shapes(world, leo70, n):
    ctx = world["ctx"]
    lib = _abi.load_library()
    traj, full = head(leo70[0], n), leo70[4]
    params = [F.X, F.Rmag, F.VY, F.PeriapsisRadius, F.C3, F.BdotT, F.BAngle, F.TrueAnomaly]
    rows = [int(p) for p in params]
    guard = 1000
    for cap in (1, TILE - 1, TILE + 1, 5 * TILE - 1, 5 * TILE + 1, 50, COUNT, COUNT + 9):
        size = 8 * cap * n
        buf = np.full(size + guard, 12345.0)
        length = np.full(n + 8, -7, dtype=np.int32)
        q = frame_query(world, world["moon"], params)
        cin = traj.as_c()
        rc = lib.nyx_hip_traj_frame_values(ctx._h, C.byref(cin), n, C.byref(q), cap, buf.ctypes.data_as(_abi.c_double_p), length.ctypes.data_as(_abi.c_int32_p))
        assert rc == 0, _abi.last_error()
        assert (length[:n] == COUNT).all() and (length[n:] == -7).all()          # produced, not stored
        vals = buf[:size].reshape(8, cap, n)
        m = min(cap, COUNT)
        np.testing.assert_array_equal(vals[:, :m], full[rows, :m, :n])           # every stored slot is the slot of test 1, bit for bit
        assert np.isnan(vals[:, m:]).all()                                       # NaN everywhere else
        assert (buf[size:] == 12345.0).all()                                      # nothing beyond n_params * capacity * n
    # positions alone - the velocity recurrence of the body is not run - and one parameter alone: the same bits
    pos, _ = ctx.traj_frame_values(traj, world["moon"], [F.Z, F.Rmag, F.X], STEP, capacity=COUNT)
    np.testing.assert_array_equal(pos, full[[int(F.Z), int(F.Rmag), int(F.X)], :, :n])
    one, _ = ctx.traj_frame_values(traj, world["moon"], [F.BdotR], STEP, capacity=COUNT)
    np.testing.assert_array_equal(one[0], full[int(F.BdotR), :, :n])


def test_5_a_sample_outside_the_ephemerides_ends_the_series(world):
    """Stored epochs that straddle the end of the Moon's chain: the series ends at the first sample past it, `len` names it, NaN
    follows; the neighbour in the same wave, a day earlier, is unaffected; seen from the centre itself (no chain) nothing ends."""
    ctx = world["ctx"]
    al = world["almanac"]
    chain = eclipse.body_chain(nx.MOON, al, world["central"])
    end_s = min(float(al.segments[s].init_et_s) + float(al.segments[s].interval_s) * al.segments[s].records.shape[0] for s, _ in chain)
    end_ns = int(end_s) * S                                # a whole second at or before the end
    k_n = 24
    t = _abi.TrajBatch(2, k_n)
    t.len[:] = k_n
    t.epoch_ns[:, 0] = end_ns - 10 * STEP + STEP * np.arange(k_n)
    t.epoch_ns[:, 1] = t.epoch_ns[:, 0] - 86400 * S
    r0, v0 = leo_nominal()[:3], leo_nominal()[3:]
    for i in range(2):
        tau = (t.epoch_ns[:, i] - t.epoch_ns[0, i]) / S
        t.state[:3, :, i] = r0[:, None] + v0[:, None] * tau[None, :]            # a straight line: any window interpolates it
        t.state[3:, :, i] = v0[:, None]
    params = [F.Rmag, F.VX, F.BdotT]
    vals, length = ctx.traj_frame_values(t, world["moon"], params, STEP, capacity=k_n + 3)
    ev = ctx.traj_every(t, STEP, k_n)
    assert (ev.len == k_n).all()                                                # every sample CAN be interpolated
    rv = np.ascontiguousarray(ev.state.transpose(1, 2, 0))
    want = host_values(world, params, rv, ev.epoch_ns, world["moon"])
    bad = np.nonzero(np.isnan(want[0, :, 0]))[0]
    assert len(bad) and 8 <= bad[0] <= 12 and not np.isnan(want[:, :, 1]).any()
    assert list(length) == [int(bad[0]), k_n]
    assert np.isfinite(vals[:, :bad[0], 0]).all() and np.isnan(vals[:, bad[0]:, 0]).all()      # later samples included
    assert np.isnan(vals[:, k_n:, 1]).all()
    assert_all_within(params, vals[:, :bad[0], :1], want[:, :bad[0], :1], label=" before the end")
    assert_all_within(params, vals[:, :k_n, 1:], want[:, :, 1:], label=" neighbour")
    own, l2 = ctx.traj_frame_values(t, world["central"], [F.Rmag], STEP)
    assert list(l2) == [k_n, k_n] and np.isfinite(own).all()


def test_6_device_pointers_on_a_stream_equal_the_host_flavour(world, leo70):
    import torch
    ctx = world["ctx"]
    lib = _abi.load_library()
    dev = torch.device("cuda", 0)
    t = leo70[0]
    n, cap, guard = t.n, 40, 512
    params = [F.Rmag, F.BdotT, F.BAngle]
    start, stop = EPOCH0_NS + 500 * S, EPOCH0_NS + 5000 * S
    host, host_len = ctx.traj_frame_values(t, world["moon"], params, STEP, start, stop, capacity=cap)
    epoch = torch.from_numpy(t.epoch_ns).to(dev)
    state = torch.from_numpy(t.state).to(dev)
    tlen = torch.from_numpy(t.len).to(dev)
    s = _abi.Traj()
    s.capacity = t.capacity
    s.epoch_ns = C.cast(epoch.data_ptr(), _abi.c_int64_p)
    for k, f in enumerate(["x_km", "y_km", "z_km", "vx_km_s", "vy_km_s", "vz_km_s"]):
        setattr(s, f, C.cast(state[k].data_ptr(), _abi.c_double_p))
    s.len = C.cast(tlen.data_ptr(), _abi.c_int32_p)
    size = 3 * cap * n
    values = torch.full((size + guard,), 12345.0, dtype=torch.float64, device=dev)
    length = torch.full((n + 8,), -7, dtype=torch.int32, device=dev)
    q = frame_query(world, world["moon"], params, start=start, stop=stop)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        rc = lib.nyx_hip_traj_frame_values_device(ctx._h, C.byref(s), n, C.byref(q), cap, C.c_void_p(values.data_ptr()), C.c_void_p(length.data_ptr()),
                                                  C.c_void_p(stream.cuda_stream))
    assert rc == 0, _abi.last_error()
    stream.synchronize()
    got, got_len = values.cpu().numpy(), length.cpu().numpy()
    np.testing.assert_array_equal(got_len[:n], host_len)
    assert (got_len[n:] == -7).all() and (host_len == 76).all()                # (5000 - 500) / 60 + 1 produced, 40 stored
    np.testing.assert_array_equal(got[:size].reshape(3, cap, n), host)
    assert (got[size:] == 12345.0).all() and np.isfinite(host).all()           # guard values: nothing beyond the buffer


def test_7_what_the_query_asks_of_the_context_is_refused_through_the_library(world, leo70):
    """A segment index beyond the context's segments: NYX_HIP_RC_BAD_ARG.  A context with an integration-frame swap:
    NYX_HIP_RC_UNSUPPORTED.  Neither launches anything: the outputs are untouched."""
    lib = _abi.load_library()
    ctx, traj = world["ctx"], head(leo70[0], 2)
    cin = traj.as_c()
    values, length = np.zeros(4 * 2), np.zeros(2, dtype=np.int32)
    vp, lp = values.ctypes.data_as(_abi.c_double_p), length.ctypes.data_as(_abi.c_int32_p)
    q = frame_query(world, world["moon"], [F.Rmag])
    q.chain_segment[1] = world["compiled"].cfg.n_segments
    assert lib.nyx_hip_traj_frame_values(ctx._h, C.byref(cin), 2, C.byref(q), 4, vp, lp) == _abi.RC_BAD_ARG
    assert "chain_segment[1]" in _abi.last_error() and "not a segment of the context" in _abi.last_error()
    swapped = nx.GpuContext(world["prop"].compile(world["almanac"], world["central"], state_frame=world["moon"]))
    try:
        q = frame_query(world, world["moon"], [F.Rmag])
        for fn, extra in ((lib.nyx_hip_traj_frame_values, ()), (lib.nyx_hip_traj_frame_values_device, (None,))):
            assert fn(swapped._h, C.byref(cin), 2, C.byref(q), 4, vp, lp, *extra) == _abi.RC_UNSUPPORTED
            assert "integration-frame swap" in _abi.last_error()
        with pytest.raises(RuntimeError, match="integration-frame swap"):
            swapped.traj_frame_values(traj, world["moon"], [F.Rmag], STEP)
    finally:
        swapped.close()
    assert (values == 0).all() and (length == 0).all()


def test_8_results_frame_values_on_a_real_monte_carlo(world):
    prop, almanac, central = world["prop"], world["almanac"], world["central"]
    template = nx.Spacecraft(EPOCH0_NS, leo_nominal(), central, dry_mass_kg=100.0, prop_mass_kg=10.0, srp_area_m2=1.0, cr=1.8)
    fail, runs = 4, 20

    class Mc(nx.MonteCarlo):
        def generate_states(self, skip, num_runs, seed=None):
            out = super().generate_states(skip, num_runs, seed)
            out[fail][1].dry_mass_kg = 0.0      # massless with a force model: that run errors
            out[fail][1].prop_mass_kg = 0.0
            return out

    mc = Mc(nx.MvnSpacecraft.from_sigmas(template, [1.0, 1.0, 1.0, 1e-3, 1e-3, 1e-3]), seed=5)
    res = mc.run_until_epoch(prop, almanac, EPOCH0_NS + DUR, runs, capacity=256)
    assert isinstance(res.runs[fail].result, nx.PropagationError) and len(res.ok_runs()) == runs - 1
    params = [F.Rmag, nx.StateParameter.PeriapsisRadius, F.C3, F.BdotT, F.BdotR]
    series = res.frame_values(world["moon"], params, STEP)
    ctx = res._traj_ctx
    assert hasattr(ctx, "traj_frame_values")

    class Compose:   # the evaluator of the definition: traj_every / traj_at only, and what the runs were compiled from
        traj_at = staticmethod(ctx.traj_at)
        traj_every = staticmethod(ctx.traj_every)
        compiled = ctx.compiled

    want = dataclasses.replace(res, _traj_ctx=Compose).frame_values(world["moon"], params, STEP)
    assert isinstance(series, nx.FrameSeries) and series.values.shape == want.values.shape == (5, COUNT, runs)
    assert series.params == [F.Rmag, F.PeriapsisRadius, F.C3, F.BdotT, F.BdotR]
    for f in ("len", "epoch0_ns", "ok"):
        np.testing.assert_array_equal(getattr(series, f), getattr(want, f))
    assert series.len[fail] == 0 and np.isnan(series.values[:, :, fail]).all() and list(np.delete(series.len, fail)) == [COUNT] * (runs - 1)
    okc = np.nonzero(series.ok)[0]
    assert_all_within(series.params, series.values[:, :, okc], want.values[:, :, okc], label=" mc")
    k, rmin = series.closest_approach()
    k2, rmin2 = want.closest_approach()
    np.testing.assert_array_equal(k, k2)
    np.testing.assert_array_equal(rmin, rmin2)
    assert k[fail] == -1 and np.isnan(rmin[fail])
    np.testing.assert_array_equal(rmin[okc], series.of(F.Rmag)[:, okc].min(axis=0))
    frac = series.hyperbolic_fraction()
    assert (frac[okc] == 1.0).all() and np.isnan(frac[fail])
    # about the Earth itself nothing is hyperbolic and every series is complete
    own = res.frame_values(central, [F.Rmag, F.BdotT], STEP)
    assert list(np.delete(own.len, fail)) == [COUNT] * (runs - 1) and (own.hyperbolic_fraction()[okc] < 0.1).all()
    np.testing.assert_array_equal(own.hyperbolic_fraction()[okc], np.isfinite(own.of(F.BdotT)[:, okc]).mean(axis=0))
    # one trajectory through Traj.frame_values, and its stored states through Traj.to_frame
    traj = res.runs[0].result.traj
    ep, one = traj.frame_values(world["moon"], series.params, STEP)
    assert list(ep) == [EPOCH0_NS + k * STEP for k in range(COUNT)] and one.shape == (5, COUNT)
    np.testing.assert_array_equal(one, series.values[:, :, 0])
    moved = traj.to_frame(world["moon"])
    np.testing.assert_array_equal(moved.epochs_ns, traj.epochs_ns)
    np.testing.assert_array_equal(moved.states, frames.to_frame(traj.states, traj.epochs_ns, world["moon"], almanac, central))
