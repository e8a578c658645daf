"""Eclipses on the MI355X (eclipse_kernel.hip, include/nyx_hip_eclipse.h).

The inertial position a value is evaluated from is the one `traj_every` / `traj_at` return (same device code), and the
ephemerides, the disk overlap and the parameters are the code tests/test_eclipse_host_cxx.py runs on the CPU against the oracle bit
for bit: the values are compared with the host definition `nyx_amd.eclipse.eclipse_value` applied to those states at their epochs,
so the only difference is the device's libm (asin, acos, sqrt, the divisions) against glibc's.  Small on purpose: at most 70
trajectories, one orbit.

THE ENSEMBLE (the fixture of tests/test_gpu_aer.py: `leo_full_setup(degree=8)`, `dispersed_leo_batch(70, seed=11)`, 5400 s, capacity
256 - one full wave plus one with 6 live lanes) starts in the Earth's umbra, leaves it through the penumbra between 1196 s and
1220 s and re-enters between 4980 s and 5002 s; the Moon never hides the Sun.  The fixtures ASSERT on the host definition what lets
the comparisons leave out NO sample: every run has lit and umbra samples, and no sample has |PenumbraMargin| or |UmbraMargin| below
1e-9 rad, so no plateau decision can flip between two libms.

TOLERANCES.  Measured on the MI355X against the host definition, per parameter, over test 1 (70 x 91 samples, two bodies) and
test 2 (70 x 181 samples across the penumbra, 17 - 18 of them inside it per run): the largest |device - eclipse_value| of the two (the
Moon's rows of test 1 included; the percentages' figure is test 2's, test 1 measured 1.2e-07).  The bound is the measured maximum x 8 rounded
up to one significant digit, and never above the ceilings, above which a deviation is a bug and not a tolerance: 1e-9 deg for the
five degree-valued parameters, 8 ulp of the value for SunRange, 1e-5 percentage points for the two percentages inside the
penumbra (about 4e-8 points per ulp of input: the conditioning of the overlap formula, acos(d / r) with d / r within 1e-5 of
1), 1e-7 for Illumination.  Plateau samples (0.0 / 100.0), State and EclipsingBody are exact.  A measured 0 stays 0: |r_ls| is
three products, two sums and a square root of the same operands on both sides, every one of them correctly rounded.

    parameter             measured    unit     bound
    Occultation           5.710e-07   points   5e-6
    Illumination          5.710e-09   -        5e-8
    State                 0           -        0
    EclipsingBody         0           -        0
    SunRange              0           ulp      0
    SunApparentRadius     5.551e-17   deg      5e-16
    BodyOccultation       5.710e-07   points   5e-6
    BodyApparentRadius    1.421e-14   deg      2e-13
    BodySeparation        2.842e-14   deg      3e-13
    BodyPenumbraMargin    4.263e-14   deg      4e-13
    BodyUmbraMargin       5.684e-14   deg      5e-13
"""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import nyx_amd as nx
from nyx_amd import _abi, eclipse
from nyx_amd.eclipse import EclipseParameter as E
from scenarios import EPOCH0_NS, dispersed_leo_batch, leo_full_setup, leo_nominal

pytestmark = pytest.mark.gpu

S = nx.NS_PER_S
STEP = 60 * S
DUR = 5400 * S
COUNT = 91
TILE = 16          # ECL_TILE of csrc/eclipse_kernel.hip
EARTH_B, MOON_B = 0, 1
MODEL_PARAMS = [E.Occultation, E.Illumination, E.State, E.EclipsingBody, E.SunRange, E.SunApparentRadius]
BODY_PARAMS = [E.BodyOccultation, E.BodyApparentRadius, E.BodySeparation, E.BodyPenumbraMargin, E.BodyUmbraMargin]
# all eleven (two launches through the Python split), the per-body ones of the Earth; then the Moon's
ALL = MODEL_PARAMS + [(p, EARTH_B) for p in BODY_PARAMS]
MOON = [(p, MOON_B) for p in BODY_PARAMS]
EXACT = (E.State, E.EclipsingBody)
DEGREES = (E.SunApparentRadius, E.BodyApparentRadius, E.BodySeparation, E.BodyPenumbraMargin, E.BodyUmbraMargin)
PERCENT = (E.Occultation, E.BodyOccultation)
# the ceilings (see above); SunRange is bounded in ulp of the value
CEILING = {**{p: 1e-9 for p in DEGREES}, **{p: 1e-5 for p in PERCENT}, E.Illumination: 1e-7, E.SunRange: 8.0, E.State: 0.0, E.EclipsingBody: 0.0}
# parameter -> bound: see the table above
TOL = {
    E.Occultation: 5e-6,
    E.Illumination: 5e-8,
    E.State: 0.0,
    E.EclipsingBody: 0.0,
    E.SunRange: 0.0,
    E.SunApparentRadius: 5e-16,
    E.BodyOccultation: 5e-6,
    E.BodyApparentRadius: 2e-13,
    E.BodySeparation: 3e-13,
    E.BodyPenumbraMargin: 4e-13,
    E.BodyUmbraMargin: 5e-13,
}


def kind(p):
    return p[0] if isinstance(p, tuple) else p


def deviation(p, got, want):
    """Largest difference of one parameter over the samples: in ulp of the value for SunRange, absolute for the others."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and np.isfinite(want).all() and np.isfinite(got).all(), kind(p).name
    if not got.size:
        return 0.0
    if kind(p) is E.SunRange:
        return float((np.abs(got - want) / np.spacing(np.abs(want))).max())
    return float(np.abs(got - want).max())


def assert_all_within(params, got, want, label=""):
    """got / want [P, ...]: every parameter over all samples inside its bound; the plateaux of the percentages exact."""
    failures = []
    for j, p in enumerate(params):
        d = deviation(p, got[j], want[j])
        print(f"deviation{label} {kind(p).name:18s} {d:.3e}  (bound {TOL[kind(p)]:.0e})")
        assert TOL[kind(p)] <= CEILING[kind(p)]
        if not d <= TOL[kind(p)]:
            failures.append(f"{kind(p).name}: {d:.3e} > {TOL[kind(p)]:.0e}")
        if kind(p) in PERCENT:
            flat = (want[j] == 0.0) | (want[j] == 100.0)
            np.testing.assert_array_equal(got[j][flat], want[j][flat])       # exactly 0.0 / 100.0
            assert ((got[j][~flat] > 0.0) & (got[j][~flat] < 100.0)).all()
        if kind(p) in EXACT:
            np.testing.assert_array_equal(got[j], want[j])
    assert not failures, "\n".join(failures)


def host_values(world, params, rv, epochs, model=None):
    """[P, ...] of the host definition."""
    model = model or world["model"]
    pairs = [p if isinstance(p, tuple) else (p, None) for p in params]
    return np.stack([nx.eclipse_value(p, rv, epochs, model, world["almanac"], world["central"], body=b) for p, b in pairs])


def assert_no_decision_can_flip(world, rv, epochs):
    """|PenumbraMargin| and |UmbraMargin| of both bodies above 1e-9 rad at every sample."""
    for b in (EARTH_B, MOON_B):
        m = host_values(world, [(E.BodyPenumbraMargin, b), (E.BodyUmbraMargin, b)], rv, epochs)
        nearest = np.abs(np.radians(m)).min()
        print(f"nearest margin of body {b}: {nearest:.3e} rad")
        assert nearest > 1e-9


@pytest.fixture(scope="module")
def world():
    prop, almanac, central = leo_full_setup(degree=8)
    compiled = prop.compile(almanac, central)
    ctx = nx.GpuContext(compiled)
    yield dict(prop=prop, almanac=almanac, central=central, compiled=compiled, ctx=ctx, model=nx.ShadowModel.cislunar(almanac))
    ctx.close()


@pytest.fixture(scope="module")
def leo70(world):
    """One orbit of 70 dispersed trajectories with dense output, its traj_every states, the host definition on those states and the
    device's eleven parameters at capacity 91: computed once, shared, never written to."""
    ctx = world["ctx"]
    _, st, traj = ctx.propagate_with_traj(dispersed_leo_batch(70, seed=11), DUR, capacity=256)
    assert (st.status == 0).all()
    ev = ctx.traj_every(traj, STEP, COUNT)
    assert (ev.len == COUNT).all()
    rv = np.ascontiguousarray(ev.state.transpose(1, 2, 0))             # [K, n, 6]
    want = host_values(world, ALL, rv, ev.epoch_ns)                     # [11, K, n]
    want_moon = host_values(world, MOON, rv, ev.epoch_ns)
    assert np.isfinite(want).all() and np.isfinite(want_moon).all()
    state = want[ALL.index(E.State)]
    print(f"samples per run: lit {(state == 0).sum(axis=0).min()} .. {(state == 0).sum(axis=0).max()}, umbra {(state == 2).sum(axis=0).min()} .. "
          f"{(state == 2).sum(axis=0).max()}, penumbra {(state == 1).sum(axis=0).min()} .. {(state == 1).sum(axis=0).max()}")
    assert ((state == 0).any(axis=0) & (state == 2).any(axis=0)).all()        # every run has lit and umbra samples
    assert (state[0] == 2).all()                                               # and starts in the umbra
    assert (want_moon[0] == 0.0).all()                                         # the Moon never hides the Sun
    assert_no_decision_can_flip(world, rv, ev.epoch_ns)
    got, length = ctx.traj_eclipse(traj, world["model"], ALL, STEP, capacity=COUNT)
    for a in (ev.state, ev.epoch_ns, rv, want, want_moon, got, length):
        a.setflags(write=False)
    return traj, ev, rv, want, want_moon, got, length


def head(traj, n):
    """The first n trajectories of a batch as a batch of their own."""
    t = _abi.TrajBatch(n, traj.capacity)
    t.epoch_ns[:], t.state[:], t.len[:] = traj.epoch_ns[:, :n], traj.state[:, :, :n], traj.len[:n]
    return t


def ecl_query(world, params, step=STEP, start=None, stop=None, model=None):
    """The query GpuContext.traj_eclipse builds, for the raw entries."""
    model = model or world["model"]
    q = _abi.EclQuery()
    q.n_params, q.step_ns, q.n_bodies = len(params), step, len(model.shadow_bodies)
    for k, p in enumerate(params):
        q.param[k], q.param_body[k] = nx.ecl_param_code(p, model)
    if start is not None:
        q.has_window, q.start_ns, q.end_ns = 1, start, stop
    for dst, frame in [(q.light, model.light_source)] + [(q.bodies[b], f) for b, f in enumerate(model.shadow_bodies)]:
        chain = eclipse.body_chain(frame.naif_id, world["almanac"], world["central"])
        dst.n_chain, dst.mean_radius_km = len(chain), float(frame.mean_equatorial_radius_km)
        for k, (seg, sign) in enumerate(chain):
            dst.chain_segment[k], dst.chain_sign[k] = seg, sign
    return q


def test_1_full_orbit_all_parameters_against_the_host_definition(world, leo70):
    traj, want, want_moon, got, length = leo70[0], leo70[3], leo70[4], leo70[5], leo70[6]
    assert set(TOL) == set(E) == set(CEILING)
    assert got.shape == (11, COUNT, 70) and length.dtype == np.int32 and (length == COUNT).all()
    assert_all_within(ALL, got, want, label=" orbit")
    moon, l2 = world["ctx"].traj_eclipse(traj, world["model"], MOON, STEP)     # capacity=None: sized from the batch's epochs
    assert moon.shape == (5, COUNT, 70) and (l2 == COUNT).all()
    assert_all_within(MOON, moon, want_moon, label=" moon")
    # the winner is the Earth wherever anything is hidden; the model's percentage is the Earth's, bit for bit
    occ = got[ALL.index(E.Occultation)]
    np.testing.assert_array_equal(got[ALL.index(E.EclipsingBody)], np.where(occ > 0.0, 0.0, -1.0))
    np.testing.assert_array_equal(occ, got[ALL.index((E.BodyOccultation, EARTH_B))])
    np.testing.assert_array_equal(got[ALL.index(E.Illumination)], np.abs(occ / 100.0 - 1.0))
    with pytest.raises(TypeError):
        world["ctx"].traj_eclipse(traj, world["model"], [E.Occultation, nx.AerParameter.Range], STEP)


def test_2_the_penumbra_resolved_across_tile_seams(world, leo70):
    ctx = world["ctx"]
    traj = leo70[0]
    start, stop = EPOCH0_NS + 1140 * S, EPOCH0_NS + 1320 * S
    q = start + S * np.arange(181, dtype=np.int64)
    states, status = ctx.traj_at(traj, q)                                       # [181, 70, 6]
    assert not _abi.interp_failed(status).any()
    epochs = np.broadcast_to(q[:, None], states.shape[:2])
    want = host_values(world, ALL, states, epochs)
    occ = want[ALL.index(E.Occultation)]
    inside = ((occ > 0.0) & (occ < 100.0)).sum(axis=0)
    print(f"penumbra samples per run: {inside.min()} .. {inside.max()}")
    assert (occ[0] == 100.0).all() and (occ[-1] == 0.0).all() and (inside >= 10).all()
    assert_no_decision_can_flip(world, states, epochs)
    got, length = ctx.traj_eclipse(traj, world["model"], ALL, S, start, stop)
    assert got.shape == (11, 181, 70) and (length == 181).all()                # 181 = 11 tiles of 16 + 5
    assert_all_within(ALL, got, want, label=" penumbra")
    assert (np.diff(got[ALL.index(E.Occultation)], axis=0) <= 1e-5).all()      # out of the shadow: never darker again


@pytest.mark.parametrize("n", [1, 64, 65])
def test_3_seams_and_shapes(world, leo70, n):
    ctx = world["ctx"]
    lib = _abi.load_library()
    traj, full = head(leo70[0], n), leo70[5]
    params = ALL[:8]
    guard = 1000
    for cap in (1, TILE - 1, TILE + 1, 5 * TILE - 1, 5 * TILE + 1, 50, COUNT, COUNT + 9):
        size = 8 * cap * n
        buf = np.full(size + guard, 12345.0)
        length = np.full(n + 8, -7, dtype=np.int32)
        q = ecl_query(world, params)
        cin = traj.as_c()
        rc = lib.nyx_hip_traj_eclipse(ctx._h, C.byref(cin), n, C.byref(q), cap, buf.ctypes.data_as(_abi.c_double_p), length.ctypes.data_as(_abi.c_int32_p))
        assert rc == 0, _abi.last_error()
        assert (length[:n] == COUNT).all() and (length[n:] == -7).all()          # produced, not stored
        vals = buf[:size].reshape(8, cap, n)
        m = min(cap, COUNT)
        np.testing.assert_array_equal(vals[:, :m], full[:8, :m, :n])             # every stored slot is the slot of test 1, bit for bit
        assert np.isnan(vals[:, m:]).all()                                       # NaN everywhere else
        assert (buf[size:] == 12345.0).all()                                      # nothing beyond n_params * capacity * n
    # the last three parameters, alone and together: the same bits
    tail, _ = ctx.traj_eclipse(traj, world["model"], ALL[8:], STEP, capacity=COUNT)
    np.testing.assert_array_equal(tail, full[8:, :, :n])
    one, _ = ctx.traj_eclipse(traj, world["model"], [ALL[9]], STEP, capacity=COUNT)
    np.testing.assert_array_equal(one[0], full[9, :, :n])


def moon_states(world):
    """The five hand-placed positions: r = p_moon + d u + off perp at EPOCH0, u the Sun -> Moon direction."""
    p_sun = eclipse.body_position(nx.SUN, np.int64(EPOCH0_NS), world["almanac"], world["central"])
    p_moon = eclipse.body_position(nx.MOON, np.int64(EPOCH0_NS), world["almanac"], world["central"])
    u = p_moon - p_sun
    u /= np.linalg.norm(u)
    perp = np.cross(u, [0, 0, 1.0])
    perp /= np.linalg.norm(perp)
    table = [(5000.0, 3.0), (5000.0, 1725.0), (5000.0, 1800.0), (450000.0, 3.0), (450000.0, 3500.0)]
    return np.array([p_moon + d * u + off * perp for d, off in table])


def test_4_hand_placed_states_the_moon_as_the_eclipsing_body(world):
    """Stored epochs = sample epochs: traj_at returns the stored states, so the hand-placed geometry reaches the second pass exactly
    as placed.  The Moon in umbra / penumbra / lit / annular / penumbra; the Earth gives 0 at all five."""
    ctx = world["ctx"]
    places = moon_states(world)
    n, k_n = len(places), 5
    t = _abi.TrajBatch(n, k_n)
    t.len[:] = k_n
    t.epoch_ns[:] = (EPOCH0_NS + STEP * np.arange(k_n))[:, None]
    for k in range(k_n):
        t.state[:3, k, :] = places.T
        t.state[3:, k, :] = 0.0
    params = MODEL_PARAMS + [(E.BodyOccultation, MOON_B), (E.BodyOccultation, EARTH_B)] + MOON[1:]
    vals, length = ctx.traj_eclipse(t, world["model"], params, STEP)
    assert vals.shape == (len(params), k_n, n) and (length == k_n).all()
    ev = ctx.traj_every(t, STEP, k_n)
    assert (ev.len == k_n).all() and np.abs(ev.state - t.state).max() < 1e-6     # (the placed states, as the device interpolates them)
    rv = np.ascontiguousarray(ev.state.transpose(1, 2, 0))
    want = host_values(world, params, rv, ev.epoch_ns)
    assert_no_decision_can_flip(world, rv[:1], ev.epoch_ns[:1])
    assert_all_within(params, vals[:, :1], want[:, :1], label=" hand-placed")   # the sample AT EPOCH0 is the placed geometry
    get = lambda p: vals[params.index(p), 0]
    moon_pct = get((E.BodyOccultation, MOON_B))
    assert moon_pct[0] == 100.0 and moon_pct[2] == 0.0
    assert np.abs(moon_pct[[1, 3, 4]] - [82.0856, 68.2198, 2.7179]).max() < 1e-4        # the CPU oracle's figures
    assert (get((E.BodyOccultation, EARTH_B)) == 0.0).all()
    np.testing.assert_array_equal(get(E.Occultation), moon_pct)
    assert list(get(E.EclipsingBody)) == [1.0, 1.0, -1.0, 1.0, 1.0] and list(get(E.State)) == [2.0, 1.0, 0.0, 1.0, 1.0]
    # annular: the Moon's disk inside the Sun's
    fo, dp, ls = get((E.BodyApparentRadius, MOON_B)), get((E.BodySeparation, MOON_B)), get(E.SunApparentRadius)
    assert fo[3] < ls[3] and dp[3] < ls[3] - fo[3] and abs(moon_pct[3] - 100.0 * (fo[3] / ls[3]) ** 2) < 1e-9
    # the body order swapped: the index follows, the values do not move
    swapped = nx.ShadowModel(world["model"].light_source, world["model"].shadow_bodies[::-1])
    sv, _ = ctx.traj_eclipse(t, swapped, [E.EclipsingBody, E.Occultation, (E.BodyOccultation, 0)], STEP)
    assert list(sv[0, 0]) == [0.0, 0.0, -1.0, 0.0, 0.0]
    np.testing.assert_array_equal(sv[1], vals[params.index(E.Occultation)])
    np.testing.assert_array_equal(sv[2], vals[params.index((E.BodyOccultation, MOON_B))])
    # the later samples: the same positions under a Sun and a Moon that have moved - still the host definition
    assert_all_within(params, vals, want, label=" hand-placed, later")


def test_5_a_sample_outside_the_ephemerides_ends_the_series(world):
    """Stored epochs that straddle the end of the almanac's shortest segment: the series ends at the first sample past it, `len`
    names it, NaN follows; the neighbour in the same wave, a day earlier, is unaffected."""
    ctx = world["ctx"]
    al = world["almanac"]
    end_s = min(float(s.init_et_s) + float(s.interval_s) * s.records.shape[0] for s in al.segments)
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
    params = [E.Occultation, E.SunRange, (E.BodySeparation, MOON_B)]
    vals, length = ctx.traj_eclipse(t, world["model"], params, STEP, capacity=k_n + 3)
    ev = ctx.traj_every(t, STEP, k_n)
    assert (ev.len == k_n).all()                                                # every sample CAN be interpolated
    rv = np.ascontiguousarray(ev.state.transpose(1, 2, 0))
    want = host_values(world, params, rv, ev.epoch_ns)
    bad = np.nonzero(np.isnan(want[:, :, 0]).any(axis=0))[0]
    assert len(bad) and 8 <= bad[0] <= 12 and not np.isnan(want[:, :, 1]).any()
    assert list(length) == [int(bad[0]), k_n]
    assert np.isfinite(vals[:, :bad[0], 0]).all() and np.isnan(vals[:, bad[0]:, 0]).all()      # later samples included
    assert np.isnan(vals[:, k_n:, 1]).all()
    assert_all_within(params, vals[:, :bad[0], :1], want[:, :bad[0], :1], label=" before the end")
    assert_all_within(params, vals[:, :k_n, 1:], want[:, :, 1:], label=" neighbour")


def test_6_device_pointers_on_a_stream_equal_the_host_flavour(world, leo70):
    import torch
    ctx = world["ctx"]
    lib = _abi.load_library()
    dev = torch.device("cuda", 0)
    t = leo70[0]
    n, cap, guard = t.n, 40, 512
    params = [E.Occultation, E.State, (E.BodyPenumbraMargin, EARTH_B)]
    start, stop = EPOCH0_NS + 500 * S, EPOCH0_NS + 5000 * S
    host, host_len = ctx.traj_eclipse(t, world["model"], params, STEP, start, stop, capacity=cap)
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
    q = ecl_query(world, params, start=start, stop=stop)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        rc = lib.nyx_hip_traj_eclipse_device(ctx._h, C.byref(s), n, C.byref(q), cap, C.c_void_p(values.data_ptr()), C.c_void_p(length.data_ptr()),
                                             C.c_void_p(stream.cuda_stream))
    assert rc == 0, _abi.last_error()
    stream.synchronize()
    got, got_len = values.cpu().numpy(), length.cpu().numpy()
    np.testing.assert_array_equal(got_len[:n], host_len)
    assert (got_len[n:] == -7).all() and (host_len == 76).all()                # (5000 - 500) / 60 + 1 produced, 40 stored
    np.testing.assert_array_equal(got[:size].reshape(3, cap, n), host)
    assert (got[size:] == 12345.0).all()                                        # guard values: nothing beyond the buffer
    assert ((host[1] == 0.0).any(axis=0) & (host[1] == 2.0).any(axis=0)).all() # the window holds the exit from the umbra


def test_7_what_the_query_asks_of_the_context_is_refused_through_the_library(world, leo70):
    """A segment index beyond the context's segments: NYX_HIP_RC_BAD_ARG.  A context with an integration-frame swap:
    NYX_HIP_RC_UNSUPPORTED.  Neither launches anything: the outputs are untouched."""
    lib = _abi.load_library()
    ctx, traj = world["ctx"], head(leo70[0], 2)
    cin = traj.as_c()
    values, length = np.zeros(4 * 2), np.zeros(2, dtype=np.int32)
    vp, lp = values.ctypes.data_as(_abi.c_double_p), length.ctypes.data_as(_abi.c_int32_p)
    q = ecl_query(world, [E.Occultation])
    q.bodies[1].chain_segment[0] = world["compiled"].cfg.n_segments
    assert lib.nyx_hip_traj_eclipse(ctx._h, C.byref(cin), 2, C.byref(q), 4, vp, lp) == _abi.RC_BAD_ARG
    assert "bodies[1].chain_segment[0]" in _abi.last_error() and "not a segment of the context" in _abi.last_error()
    moon_frame = world["almanac"].frame_info(nx.MOON)
    swapped = nx.GpuContext(world["prop"].compile(world["almanac"], world["central"], state_frame=moon_frame))
    try:
        q = ecl_query(world, [E.Occultation])
        for fn, extra in ((lib.nyx_hip_traj_eclipse, ()), (lib.nyx_hip_traj_eclipse_device, (None,))):
            assert fn(swapped._h, C.byref(cin), 2, C.byref(q), 4, vp, lp, *extra) == _abi.RC_UNSUPPORTED
            assert "integration-frame swap" in _abi.last_error()
        with pytest.raises(RuntimeError, match="integration-frame swap"):
            swapped.traj_eclipse(traj, world["model"], [E.Occultation], STEP)
    finally:
        swapped.close()
    assert (values == 0).all() and (length == 0).all()


def test_8_results_eclipses_on_a_real_monte_carlo(world):
    prop, almanac, central = world["prop"], world["almanac"], world["central"]
    model = world["model"]
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
    params = [E.Occultation, E.State, E.EclipsingBody, (E.BodyPenumbraMargin, model.shadow_bodies[0])]
    series = res.eclipses(model, STEP, params)
    ctx = res._traj_ctx
    assert hasattr(ctx, "traj_eclipse")

    class Compose:   # the evaluator of the definition: traj_every / traj_at only, and what the runs were compiled from
        traj_at = staticmethod(ctx.traj_at)
        traj_every = staticmethod(ctx.traj_every)
        compiled = ctx.compiled

    want = dataclasses.replace(res, _traj_ctx=Compose).eclipses(model, STEP, params)
    assert isinstance(series, nx.EclipseSeries) and series.values.shape == want.values.shape == (4, COUNT, runs)
    np.testing.assert_array_equal(series.len, want.len)
    np.testing.assert_array_equal(series.epoch0_ns, want.epoch0_ns)
    np.testing.assert_array_equal(series.ok, want.ok)
    assert series.len[fail] == 0 and np.isnan(series.values[:, :, fail]).all() and list(np.delete(series.len, fail)) == [COUNT] * (runs - 1)
    okc = np.nonzero(series.ok)[0]
    margins = np.abs(np.radians(want.values[3][:, okc]))
    assert margins.min() > 1e-9
    assert_all_within([E.Occultation, E.State, E.EclipsingBody, (E.BodyPenumbraMargin, 0)], series.values[:, :, okc], want.values[:, :, okc], label=" mc")
    # the figures of the series equal the same figures formed from the host definition
    for name in ("shadow_fraction", "umbra_fraction", "state_changes"):
        a, b = getattr(series, name), getattr(want, name)
        np.testing.assert_array_equal(a[okc], b[okc], err_msg=name)
    assert np.isnan(series.shadow_fraction[fail]) and series.state_changes[fail] == 0
    assert ((series.shadow_fraction[okc] > 0.25) & (series.shadow_fraction[okc] < 0.4)).all()       # 27-28 umbra + 1-2 penumbra of 91
    assert (series.umbra_fraction[okc] <= series.shadow_fraction[okc]).all()
    assert ((series.state_changes[okc] >= 2) & (series.state_changes[okc] <= 6)).all()               # out of the umbra, back into it
    # one trajectory through Traj.eclipse: the default set is the percentage and the state
    ep, one = res.runs[0].result.traj.eclipse(model, STEP)
    assert list(ep) == [EPOCH0_NS + k * STEP for k in range(COUNT)] and one.shape == (2, COUNT)
    np.testing.assert_array_equal(one, series.values[:2, :, 0])
