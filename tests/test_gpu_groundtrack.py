"""Ground tracks on the MI355X (groundtrack_kernel.hip, include/nyx_hip_groundtrack.h).

The inertial state a value is evaluated from is the one `traj_every` / `traj_at` return (same device code), so with
`frame.rotation None` X .. VZ must come back BIT-IDENTICAL; in a rotating frame the values are compared with the host
definition `nyx_amd.groundtrack.ground_track_value` applied to those states at their epochs, so the only difference is the
device's libm (sincos, atan2, sin, asin, sqrt) against glibc's.  Small on purpose: at most 70 trajectories, one orbit.

TOLERANCES (test 2).  Measured on the MI355X (70 dispersed LEO trajectories, one orbit, one sample per 60 s = 6 370 samples
per parameter, IAU_EARTH with a = 6378.1363 km, f = 1 / 298.257): the largest |device - ground_track_value|, in degrees
(difference wrapped to [-180, 180)) for the angles, in km or km/s for the others.  The bound is the measured figure x 8
rounded up to one significant digit - the run is deterministic, the margin covers a compiler or libm change of a few ulp -
and never above the ceilings 1e-9 deg / 1e-9 km (km/s), roughly 0.1 mm on the ground: a deviation above the ceiling is a bug,
not a tolerance.  A measured 0 stays 0.  The windows, the backward batch and the Monte Carlo (tests 5, 8, 11) are orbit samples
of the same kind, measure no more than these figures, and use this table.

    parameter      measured    unit   bound
    Latitude       0           deg    0
    Longitude      5.684e-14   deg    5e-13
    Height         4.547e-12   km     4e-11
    Rmag           1.819e-12   km     2e-11
    Declination    2.842e-14   deg    3e-13
    X              9.095e-13   km     8e-12
    Y              9.095e-13   km     8e-12
    Z              0           km     0
    VX             3.053e-16   km/s   3e-15
    VY             1.776e-15   km/s   2e-14
    VZ             0           km/s   0
    Vmag           1.776e-15   km/s   2e-14

The hand-placed states of test 4 use the same table but for ONE row, Height, which has a bound of its own (TOL_EXACT): at a
geocentric latitude of 89.9 deg `ev_geodetic` takes the height from r_delta / cos(lat) (its near-pole branch starts only at
|cos(lat)| <= 1e-6), which multiplies the last bit of the device's cos by (N + h) tan(lat) = 6 778 km x 573 = 3.9e6 km.  Measured
there: 8.740e-10 km, two half-ulps of cos, with the latitude itself equal to the last bit; x 8 of it is above the ceiling, so the
bound is the ceiling, 1e-9 km.  The margin is 14 %: should a libm or compiler change move the device's cos by one more ulp at that
state, this row fails, and the failure then points at the conditioning of the non-polar branch of `ev_geodetic` (event_dev.h, shared
with the stop conditions), not at the ground-track kernel - the state is where the issue asks for it, lat 89.9 deg.

The Moon (test 3: n = 65, two-body low lunar orbit, IAU_MOON with its 13 terms) under the same rule:

    parameter      measured    unit   bound
    Latitude       0           deg    0
    Longitude      5.684e-14   deg    5e-13
    Height         1.592e-12   km     2e-11
    Rmag           9.095e-13   km     8e-12
"""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import nyx_amd as nx
from nyx_amd import _abi, ephem
from nyx_amd.groundtrack import GroundTrackParameter as G, ground_track_value
from scenarios import EPOCH0_NS, dispersed_leo_batch, keplerian_to_cartesian, leo_full_setup, leo_nominal, two_body_setup

pytestmark = pytest.mark.gpu

S = nx.NS_PER_S
STEP = 60 * S
DUR = 5400 * S
COUNT = 91
A_KM, F = 6378.1363, 1.0 / 298.257
IAU_EARTH = nx.Frame(nx.EARTH, ephem.MU_EARTH, A_KM, nx.IAU_EARTH_ROTATION, F)
INERTIAL = nx.Frame(nx.EARTH, ephem.MU_EARTH, A_KM, None, F)
IAU_MOON = nx.Frame(nx.MOON, ephem.MU_MOON, ephem.R_MOON, nx.IAU_MOON_ROTATION, 0.0)
CART = [G.X, G.Y, G.Z, G.VX, G.VY, G.VZ]
ALL = list(G)
ANGLES = {G.Latitude, G.Longitude, G.Declination}
CEILING = 1e-9     # deg for the angles, km or km/s for the others
# parameter -> bound: see the table above
TOL = {
    G.Latitude: 0.0,
    G.Longitude: 5e-13,
    G.Height: 4e-11,
    G.Rmag: 2e-11,
    G.Declination: 3e-13,
    G.X: 8e-12,
    G.Y: 8e-12,
    G.Z: 0.0,
    G.VX: 3e-15,
    G.VY: 2e-14,
    G.VZ: 0.0,
    G.Vmag: 2e-14,
}
# test 4, the hand-placed states: test 2's bounds, but for the height at lat 89.9 deg (8.740e-10 km measured, x 8 is above the
# ceiling: the ceiling; r_delta / cos(lat) of ev_geodetic, see above)
TOL_EXACT = dict(TOL)
TOL_EXACT[G.Height] = CEILING
TOL_MOON = {
    G.Latitude: 0.0,
    G.Longitude: 5e-13,
    G.Height: 2e-11,
    G.Rmag: 8e-12,
}


def deviation(p, got, want):
    """Largest difference of one parameter over the samples: wrapped degrees for the angles, absolute for the others."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and np.isfinite(want).all() and np.isfinite(got).all(), p.name
    if not got.size:
        return 0.0
    if p in ANGLES:
        return float(np.abs((got - want + 180.0) % 360.0 - 180.0).max())
    return float(np.abs(got - want).max())


def assert_within(p, got, want, tol=None, label=""):
    tol = TOL if tol is None else tol
    d = deviation(p, got, want)
    print(f"deviation{label} {p.name:12s} {d:.3e}  (bound {tol[p]:.0e})")
    assert tol[p] <= CEILING
    assert d <= tol[p], f"{p.name}: {d:.3e} > {tol[p]:.0e}"


def assert_all_within(params, got, want, tol=None, label=""):
    failures = []
    for j, p in enumerate(params):
        try:
            assert_within(p, got[j], want[j], tol, label)
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, "\n".join(failures)


@pytest.fixture(scope="module")
def leo():
    prop, almanac, central = leo_full_setup(degree=8)
    compiled = prop.compile(almanac, central)
    ctx = nx.GpuContext(compiled)
    yield prop, almanac, central, compiled, ctx
    ctx.close()


@pytest.fixture(scope="module")
def leo70(leo):
    """One orbit of 70 dispersed trajectories with dense output, its traj_every states and the host definition on them: computed
    once, shared, never written to."""
    ctx = leo[4]
    _, st, traj = ctx.propagate_with_traj(dispersed_leo_batch(70, seed=11), DUR, capacity=256)
    assert (st.status == 0).all()
    ev = ctx.traj_every(traj, STEP, COUNT)
    assert (ev.len == COUNT).all()
    rv = np.ascontiguousarray(ev.state.transpose(1, 2, 0))             # [K, n, 6]
    want = np.stack([ground_track_value(p, rv, ev.epoch_ns, IAU_EARTH) for p in ALL])
    for a in (ev.state, ev.epoch_ns, rv, want):
        a.setflags(write=False)
    return traj, ev, rv, want


def head(traj, n):
    """The first n trajectories of a batch as a batch of their own."""
    t = _abi.TrajBatch(n, traj.capacity)
    t.epoch_ns[:], t.state[:], t.len[:] = traj.epoch_ns[:, :n], traj.state[:, :, :n], traj.len[:n]
    return t


def host_series(ctx, traj, frame, params, start=None, stop=None, step=STEP):
    """The host composition per run: (values[P, K, n] NaN-padded, len[n], first[n]) from traj_at + ground_track_value."""
    lo, hi = nx.series_bounds(traj, start, stop)
    counts = np.where(hi >= lo, (hi - lo) // step + 1, 0)
    k_max = int(counts.max()) if len(counts) else 0
    out = np.full((len(params), k_max, traj.n), np.nan)
    for i in range(traj.n):
        if counts[i] == 0:
            continue
        q = int(lo[i]) + step * np.arange(int(counts[i]), dtype=np.int64)
        states, status = ctx.traj_at(head_one(traj, i), q)
        assert not _abi.interp_failed(status).any()
        for j, p in enumerate(params):
            out[j, :counts[i], i] = ground_track_value(p, states[:, 0], q, frame)
    return out, counts.astype(np.int32), lo


def head_one(traj, i):
    t = _abi.TrajBatch(1, traj.capacity)
    t.epoch_ns[:, 0], t.state[:, :, 0], t.len[0] = traj.epoch_ns[:, i], traj.state[:, :, i], traj.len[i]
    return t


@pytest.mark.parametrize("n", [1, 64, 65, 70])
def test_1_cartesian_without_a_rotation_is_traj_every_bit_for_bit(leo, leo70, n):
    ctx = leo[4]
    traj, ev = head(leo70[0], n), leo70[1]
    for cap in (15, 16, 17, 91, 100):
        vals, length = ctx.traj_ground_track(traj, INERTIAL, CART, STEP, capacity=cap)
        assert vals.shape == (6, cap, n) and length.dtype == np.int32 and (length == COUNT).all()
        m = min(COUNT, cap)
        np.testing.assert_array_equal(vals[:, :m], ev.state[:, :m, :n])        # bit for bit
        assert np.isnan(vals[:, m:]).all()                                     # the kernel blanks what it did not produce
    v2, l2 = ctx.traj_ground_track(traj, INERTIAL, CART, STEP)                 # capacity=None: sized from the batch's epochs
    assert v2.shape == (6, COUNT, n)
    np.testing.assert_array_equal(v2, ev.state[:, :, :n])


@pytest.mark.parametrize("n", [1, 64, 65, 70])
def test_2_all_parameters_against_the_host_definition(leo, leo70, n):
    ctx = leo[4]
    traj, want = head(leo70[0], n), leo70[3]
    assert set(TOL) == set(ALL)
    for cap in ((15, 16, 17, 91, 100) if n == 70 else (91,)):
        vals, length = ctx.traj_ground_track(traj, IAU_EARTH, ALL, STEP, capacity=cap)      # twelve parameters: two launches
        assert vals.shape == (12, cap, n) and (length == COUNT).all()
        m = min(COUNT, cap)
        assert np.isnan(vals[:, m:]).all()
        assert_all_within(ALL, vals[:, :m], want[:, :m, :n], label=f" n={n} cap={cap}")
    lon = vals[ALL.index(G.Longitude), :m]
    assert (lon >= 0.0).all() and (lon < 360.0).all()


def test_3_moon_with_its_thirteen_terms():
    prop, almanac, _ = two_body_setup(nx.IntegratorMethod.DormandPrince78, nx.IntegratorOptions(), ephem.MU_MOON)
    central = nx.Frame(nx.MOON, ephem.MU_MOON, ephem.R_MOON, None)
    ctx = nx.GpuContext(prop.compile(almanac, central))
    nominal = keplerian_to_cartesian(ephem.R_MOON + 50.0, 0.002, 89.5, 30.0, 0.0, 40.0, ephem.MU_MOON)
    rng = np.random.default_rng(4)
    b = _abi.StateBatch(65)
    b.set_rv(nominal[None, :] + rng.standard_normal((65, 6)) * np.array([0.1, 0.1, 0.1, 1e-4, 1e-4, 1e-4]))
    b.epoch_ns[:] = EPOCH0_NS
    b.dry_mass_kg[:] = 1000.0
    _, st, traj = ctx.propagate_with_traj(b, 7200 * S, capacity=400)
    assert (st.status == 0).all()
    params = [G.Latitude, G.Longitude, G.Height, G.Rmag]
    ev = ctx.traj_every(traj, STEP, 121)
    vals, length = ctx.traj_ground_track(traj, IAU_MOON, params, STEP, capacity=121)
    ctx.close()
    assert (length == 121).all() and (ev.len == 121).all()
    rv = np.ascontiguousarray(ev.state.transpose(1, 2, 0))
    want = np.stack([ground_track_value(p, rv, ev.epoch_ns, IAU_MOON) for p in params])
    assert set(TOL_MOON) == set(params)
    assert_all_within(params, vals, want, TOL_MOON, label=" moon")
    h = vals[2]
    assert 40.0 < h.min() and h.max() < 60.0 and np.abs(vals[0]).max() > 60.0       # 50 km above the sphere, polar about the EARTH's pole: up to 71 deg of lunar latitude
    # a frame of another centre is refused
    earth_ctx_frame = nx.Frame(nx.EARTH, ephem.MU_EARTH, A_KM, nx.IAU_EARTH_ROTATION, F)
    ctx2 = nx.GpuContext(prop.compile(almanac, central))
    with pytest.raises(NotImplementedError, match="same centre"):
        ctx2.traj_ground_track(traj, earth_ctx_frame, params, STEP)
    ctx2.close()


def test_4_exact_hits_at_hand_placed_states(leo):
    """Stored epochs ARE the sample epochs: traj_at returns the stored states without interpolating."""
    ctx = leo[4]
    m, _ = nx.iau_dcm(nx.IAU_EARTH_ROTATION, EPOCH0_NS)
    r = A_KM + 400.0
    lat = np.radians(89.9)
    fixed = np.array([[0.0, 0.0, r], [0.0, 0.0, -r],                                      # over the poles (x = y = 0)
                      [r, 0.0, 0.0], [r, -0.0, 0.0], [-r, 0.0, 0.0], [-r, -0.0, 0.0],     # on the equator at y = +-0
                      [r, 1e-6, 10.0], [r, -1e-6, 10.0],                                  # either side of the 0 / 360 wrap
                      [r * np.cos(lat), 0.0, r * np.sin(lat)], [0.0, -r * np.cos(lat), -r * np.sin(lat)]])   # latitude +-89.9 deg
    n, k_n = len(fixed), 5
    t = _abi.TrajBatch(n, k_n)
    t.len[:] = k_n
    t.epoch_ns[:] = (EPOCH0_NS + STEP * np.arange(k_n))[:, None]
    for k in range(k_n):
        t.state[:3, k, :] = fixed.T
        t.state[3:, k, :] = np.array([0.3, -7.0, 1.0])[:, None]
    # without a rotation the hand-placed components reach the formulas exactly as placed
    params = [G.Latitude, G.Longitude, G.Height, G.Rmag, G.Declination, G.X, G.Y, G.Vmag]
    vals, length = ctx.traj_ground_track(t, INERTIAL, params, STEP)
    assert (length == k_n).all() and vals.shape == (8, k_n, n)
    rv = np.ascontiguousarray(t.state.transpose(1, 2, 0))
    want = np.stack([ground_track_value(p, rv, t.epoch_ns, INERTIAL) for p in params])
    off_pole = np.arange(n) >= 2
    for j, p in enumerate(params):
        cols = off_pole if p is G.Longitude else np.ones(n, dtype=bool)     # longitude is not compared at the exact pole
        assert_within(p, vals[j][:, cols], want[j][:, cols], TOL_EXACT, label=" exact")
    lon = vals[1]
    assert (lon[:, 2] == 0.0).all() and (lon[:, 3] == 0.0).all() and (lon[:, 4] == 180.0).all() and (lon[:, 5] == 180.0).all()
    assert (lon[:, 6] > 0.0).all() and (lon[:, 6] < 1e-6).all() and (lon[:, 7] > 359.999999).all() and (lon[:, 7] < 360.0).all()
    assert (lon[:, 2:] >= 0.0).all() and (lon[:, 2:] < 360.0).all()
    assert np.abs(vals[0][:, 0] - 90.0).max() < 1e-12 and np.abs(vals[0][:, 1] + 90.0).max() < 1e-12
    assert np.abs(np.abs(vals[0][:, 8:]) - 89.9).max() < 0.2             # (geocentric 89.9 deg: geodetic a little closer to the pole)
    # in the rotating frame: the same places expressed inertially at each stored epoch, device against host definition
    for k in range(k_n):
        mk, _ = nx.iau_dcm(nx.IAU_EARTH_ROTATION, int(t.epoch_ns[k, 0]))
        t.state[:3, k, :] = mk.T @ fixed.T
    vals, length = ctx.traj_ground_track(t, IAU_EARTH, params, STEP)
    rv = np.ascontiguousarray(t.state.transpose(1, 2, 0))
    want = np.stack([ground_track_value(p, rv, t.epoch_ns, IAU_EARTH) for p in params])
    for j, p in enumerate(params):
        cols = off_pole if p is G.Longitude else np.ones(n, dtype=bool)
        assert_within(p, vals[j][:, cols], want[j][:, cols], TOL_EXACT, label=" exact, rotating")


def test_5_windows_against_the_host_composition(leo, leo70):
    ctx = leo[4]
    traj = head(leo70[0], 65)
    end = EPOCH0_NS + DUR
    params = [G.Latitude, G.Longitude, G.Height, G.Rmag, G.VX]
    windows = [(EPOCH0_NS + 777 * S, EPOCH0_NS + 3000 * S + 5, 38),      # clips both ends
               (EPOCH0_NS - 1000 * S, EPOCH0_NS + 2000 * S, 34),          # clips the end only (the start is clamped to the first epoch)
               (EPOCH0_NS - STEP, end + STEP, 91),                        # clips nothing
               (end + S, end + 100 * S, 0)]                               # empty: after the runs
    for start, stop, count in windows:
        vals, length = ctx.traj_ground_track(traj, IAU_EARTH, params, STEP, start, stop)
        want, want_len, first = host_series(ctx, traj, IAU_EARTH, params, start, stop)
        np.testing.assert_array_equal(length, want_len)
        assert (length == count).all() and vals.shape == (5, max(count, 1), 65)
        if count:
            assert (first == max(start, EPOCH0_NS)).all()
            assert_all_within(params, vals, want, label=f" window {count}")
        else:
            assert np.isnan(vals).all()


def test_6_capacity_below_the_produced_count(leo, leo70):
    ctx = leo[4]
    lib = _abi.load_library()
    traj = leo70[0]
    n, cap, guard = traj.n, 50, 1000
    full, _ = ctx.traj_ground_track(traj, IAU_EARTH, [G.Latitude, G.Height], STEP, capacity=COUNT)
    buf = np.full(2 * cap * n + guard, 12345.0)
    length = np.full(n + 8, -7, dtype=np.int32)
    q = _abi.GtQuery()
    q.n_params, q.step_ns = 2, STEP
    q.param[0], q.param[1] = _abi.GT_PARAM["Latitude"], _abi.GT_PARAM["Height"]
    nx.fill_gt_frame(q, IAU_EARTH)
    cin = traj.as_c()
    rc = lib.nyx_hip_traj_ground_track(ctx._h, C.byref(cin), n, C.byref(q), cap, buf.ctypes.data_as(_abi.c_double_p), length.ctypes.data_as(_abi.c_int32_p))
    assert rc == 0, _abi.last_error()
    assert (length[:n] == COUNT).all() and (length[n:] == -7).all()          # produced, not stored
    np.testing.assert_array_equal(buf[: 2 * cap * n].reshape(2, cap, n), full[:, :cap])
    assert (buf[2 * cap * n:] == 12345.0).all()                               # nothing beyond n_params * capacity * n


def test_7_eight_in_one_launch_equal_eight_launches_and_the_split_of_nine(leo, leo70):
    ctx = leo[4]
    traj = leo70[0]
    eight = [G.Latitude, G.Longitude, G.Height, G.Rmag, G.Declination, G.X, G.VY, G.Vmag]
    together, ln = ctx.traj_ground_track(traj, IAU_EARTH, eight, STEP, capacity=COUNT)
    for j, p in enumerate(eight):
        alone, l1 = ctx.traj_ground_track(traj, IAU_EARTH, [p], STEP, capacity=COUNT)
        np.testing.assert_array_equal(alone[0], together[j], err_msg=p.name)
        np.testing.assert_array_equal(l1, ln)
    nine = eight + [G.Z]
    split, l9 = ctx.traj_ground_track(traj, IAU_EARTH, nine, STEP, capacity=COUNT)
    assert split.shape == (9, COUNT, traj.n)
    np.testing.assert_array_equal(split[:8], together)
    np.testing.assert_array_equal(split[8], ctx.traj_ground_track(traj, IAU_EARTH, [G.Z], STEP, capacity=COUNT)[0][0])
    np.testing.assert_array_equal(l9, ln)
    with pytest.raises(TypeError):
        ctx.traj_ground_track(traj, IAU_EARTH, [G.X, nx.StateParameter.Cr], STEP)


def test_8_back_propagated_batch(leo):
    ctx = leo[4]
    b = dispersed_leo_batch(65, seed=31)
    out, st, back = ctx.propagate_with_traj(b, -DUR, capacity=200)
    assert (st.status == 0).all() and back.epoch_ns[1, 0] < back.epoch_ns[0, 0]
    ev = ctx.traj_every(back, STEP, 96)
    cart, length = ctx.traj_ground_track(back, INERTIAL, CART, STEP, capacity=96)
    assert (length == COUNT).all() and (ev.len == COUNT).all()
    np.testing.assert_array_equal(cart[:, :COUNT], ev.state[:, :COUNT])
    assert np.isnan(cart[:, COUNT:]).all()
    np.testing.assert_array_equal(cart[:, 0, :], out.rv().T)          # the series starts at the EARLIEST epoch: the end state
    np.testing.assert_array_equal(cart[:, 90, :], b.rv().T)
    params = [G.Latitude, G.Longitude, G.Height, G.Rmag]
    vals, l2 = ctx.traj_ground_track(back, IAU_EARTH, params, STEP, capacity=96)
    np.testing.assert_array_equal(l2, length)
    rv = np.ascontiguousarray(ev.state[:, :COUNT].transpose(1, 2, 0))
    assert (ev.epoch_ns[:COUNT, 0] == EPOCH0_NS - DUR + STEP * np.arange(COUNT)).all()
    want = np.stack([ground_track_value(p, rv, ev.epoch_ns[:COUNT], IAU_EARTH) for p in params])
    assert_all_within(params, vals[:, :COUNT], want, label=" backward")


def test_9_device_pointers_on_a_stream_equal_the_host_flavour(leo, leo70):
    import torch
    ctx = leo[4]
    lib = _abi.load_library()
    dev = torch.device("cuda", 0)
    t = leo70[0]
    n, cap, guard = t.n, 40, 512
    params = [G.Latitude, G.Longitude, G.Height]
    start, stop = EPOCH0_NS + 500 * S, EPOCH0_NS + 5000 * S
    host, host_len = ctx.traj_ground_track(t, IAU_EARTH, params, STEP, start, stop, capacity=cap)
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
    q = _abi.GtQuery()
    q.n_params, q.has_window, q.step_ns, q.start_ns, q.end_ns = 3, 1, STEP, start, stop
    for k, p in enumerate(params):
        q.param[k] = _abi.GT_PARAM[p.name]
    nx.fill_gt_frame(q, IAU_EARTH)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        rc = lib.nyx_hip_traj_ground_track_device(ctx._h, C.byref(s), n, C.byref(q), cap, C.c_void_p(values.data_ptr()), C.c_void_p(length.data_ptr()),
                                                  C.c_void_p(stream.cuda_stream))
    assert rc == 0, _abi.last_error()
    stream.synchronize()
    got, got_len = values.cpu().numpy(), length.cpu().numpy()
    np.testing.assert_array_equal(got_len[:n], host_len)
    assert (got_len[n:] == -7).all() and (host_len == 76).all()                # (5000 - 500) / 60 + 1 produced, 40 stored
    np.testing.assert_array_equal(got[: 3 * cap * n].reshape(3, cap, n), host)
    assert (got[3 * cap * n:] == 12345.0).all()                                 # guard values: nothing beyond the buffer


def test_10_the_series_ends_at_the_first_sample_that_cannot_be_interpolated(leo):
    """Two stored states 10 ns apart are the same f64 second: InterpMath for every window that holds them.  The series of that
    trajectory ends there (traj_it.rs:39-61), as nyx_hip_traj_every reports, and what later chunks could interpolate again is
    blanked (the trajectory of the last test of tests/test_gpu_reports.py)."""
    ctx = leo[4]
    rng = np.random.default_rng(9)
    t = _abi.TrajBatch(2, 20)
    t.len[:] = 20
    for i in range(2):
        t.epoch_ns[:, i] = EPOCH0_NS + i * 13 + np.cumsum(rng.integers(5, 120, size=20)) * 10**9 + rng.integers(0, 10**9, size=20)
    t.state[:] = rng.standard_normal(t.state.shape) * 7000.0
    t.epoch_ns[8, 1] = t.epoch_ns[7, 1] + 10
    ev = ctx.traj_every(t, 10**9, 4096)
    vals, length = ctx.traj_ground_track(t, IAU_EARTH, [G.Latitude, G.Rmag], 10**9, capacity=4096)
    cart, cl = ctx.traj_ground_track(t, INERTIAL, [G.X], 10**9, capacity=4096)
    np.testing.assert_array_equal(length, ev.len)
    np.testing.assert_array_equal(cl, ev.len)
    assert 0 < length[1] < length[0]             # trajectory 1 ends early: its first windows hold the coincident pair
    for i in range(2):
        m = int(length[i])
        np.testing.assert_array_equal(cart[0, :m, i], ev.state[0, :m, i])
        assert np.isfinite(vals[:, :m, i]).all() and np.isnan(vals[:, m:, i]).all() and np.isnan(cart[:, m:, i]).all()
    first1 = int(t.epoch_ns[0, 1])
    k_late = int((t.epoch_ns[17, 1] - first1) // 10**9) + 1
    at, status = ctx.traj_at(t, [first1 + k_late * 10**9])
    assert status[0, 1] == _abi.INTERP_OK and np.isfinite(at[0, 1]).all() and k_late > 16 + length[1]
    assert np.isnan(vals[:, k_late, 1]).all()


def test_11_results_ground_tracks_on_a_real_monte_carlo(leo):
    prop, almanac, central = leo[:3]
    template = nx.Spacecraft(EPOCH0_NS, leo_nominal(), central, dry_mass_kg=100.0, prop_mass_kg=10.0, srp_area_m2=1.0, cr=1.8)
    fail = 4

    class Mc(nx.MonteCarlo):
        def generate_states(self, skip, num_runs, seed=None):
            out = super().generate_states(skip, num_runs, seed)
            out[fail][1].dry_mass_kg = 0.0      # massless with a force model: that run errors
            out[fail][1].prop_mass_kg = 0.0
            return out

    mc = Mc(nx.MvnSpacecraft.from_sigmas(template, [1.0, 1.0, 1.0, 1e-3, 1e-3, 1e-3]), seed=5)
    res = mc.run_until_epoch(prop, almanac, EPOCH0_NS + DUR, 70, capacity=256)
    assert isinstance(res.runs[fail].result, nx.PropagationError) and len(res.ok_runs()) == 69
    nine = [G.Latitude, G.Longitude, G.Height, G.Rmag, G.Declination, G.X, G.VY, G.Vmag, G.Z]
    gs = res.ground_tracks(IAU_EARTH, STEP, nine)
    ctx = res._traj_ctx
    assert hasattr(ctx, "traj_ground_track")

    class Compose:   # the evaluator of the definition: traj_every / traj_at only
        traj_at = staticmethod(ctx.traj_at)
        traj_every = staticmethod(ctx.traj_every)

    want = dataclasses.replace(res, _traj_ctx=Compose).ground_tracks(IAU_EARTH, STEP, nine)
    assert gs.values.shape == want.values.shape == (9, COUNT, 70)
    np.testing.assert_array_equal(gs.len, want.len)
    np.testing.assert_array_equal(gs.epoch0_ns, want.epoch0_ns)
    np.testing.assert_array_equal(gs.ok, want.ok)
    assert gs.len[fail] == 0 and np.isnan(gs.values[:, :, fail]).all() and list(np.delete(gs.len, fail)) == [COUNT] * 69
    assert list(gs.epochs(0)) == [EPOCH0_NS + k * STEP for k in range(COUNT)] and len(gs.epochs(fail)) == 0
    okc = np.nonzero(gs.ok)[0]
    assert_all_within(nine, gs.values[:, :, okc], want.values[:, :, okc], label=" mc")
    # one trajectory through Traj.ground_track: the default set is the reference's four fields
    ep, one = res.runs[0].result.traj.ground_track(IAU_EARTH, STEP)
    assert list(ep) == [EPOCH0_NS + k * STEP for k in range(COUNT)] and one.shape == (4, COUNT)
    np.testing.assert_array_equal(one, gs.values[:4, :, 0])


def test_12_height_at_the_stop_condition_is_the_events_height():
    """A run stopped by until_event(Height = h) in the same frame reports h at the event epoch, within the event's precision
    (the set-up of tests/test_gpu_events.py: two-body, DormandPrince78, the pck08-shaped IAU Earth)."""
    shaped = nx.Frame(nx.EARTH, ephem.MU_EARTH, 6378.14, nx.IAU_EARTH_ROTATION, flattening=(6378.14 - 6356.75) / 6378.14)
    prop, almanac, central = two_body_setup(nx.IntegratorMethod.DormandPrince78, nx.IntegratorOptions(), ephem.MU_EARTH)
    b = dispersed_leo_batch(1, seed=31)
    sc = nx.Spacecraft(EPOCH0_NS, b.rv()[0], central, dry_mass_kg=100.0)
    h, precision = 330.0, 1e-7
    ev = nx.Event(_abi.EV_HEIGHT_KM, h, value_precision=precision, frame=shaped)
    state, traj = prop.with_(sc, almanac).until_event(4 * 3600 * S, ev)
    assert traj.start_epoch() == EPOCH0_NS < state.epoch_ns <= traj.end_epoch()
    ep, vals = traj.ground_track(shaped, STEP, [G.Height, G.Latitude], state.epoch_ns, state.epoch_ns)
    assert list(ep) == [state.epoch_ns] and vals.shape == (2, 1)
    print(f"height at the event: {vals[0, 0]!r} (desired {h}, value_precision {precision})")
    assert abs(vals[0, 0] - h) <= precision
    # and along the whole track the last sample of the full series approaches it from the start height
    ep_all, all_h = traj.ground_track(shaped, STEP, [G.Height])
    assert ep_all[0] == EPOCH0_NS and np.isfinite(all_h).all()
