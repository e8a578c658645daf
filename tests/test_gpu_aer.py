"""Station views on the MI355X (aer_kernel.hip, include/nyx_hip_aer.h).

The inertial state a value is evaluated from is the one `traj_every` / `traj_at` return (same device code), and the constants of a
station are computed on the host by the C function the Python definition restates bit for bit (tests/test_aer_host_cxx.py): the
values are compared with the host definition `nyx_amd.stations.aer_value` applied to those states at their epochs, so the only
difference is the device's libm (sincos, asin, atan2, sqrt) against glibc's on the per-sample part.  Small on purpose: at most 70
trajectories, one orbit.

THE STATIONS are derived in the fixture from the host ground track of run 0 at sample 20: A half a degree of latitude north of that
point, B half a degree south, both 0.5 km above the ellipsoid with a mask of 5 deg in IAU_EARTH.  Every run then passes both (a
handful of visible samples, more than eighty invisible ones), no sample is nearer than 1 km to a station's zenith line (where the
azimuth loses its meaning) and none sits on the mask: the fixture ASSERTS these on the host definition of the real trajectories -
both values of `Visible` for every run and station, a horizontal range above 1 km, |elevation - mask| above 1e-6 deg - and the
comparisons leave out NO sample.

TOLERANCES (test 1).  Measured on the MI355X (70 dispersed LEO trajectories, one orbit, one sample per 60 s, two stations =
12 740 samples per parameter, IAU_EARTH with a = 6378.1363 km, f = 1 / 298.257): the largest |device - aer_value|, in degrees
(difference wrapped to [-180, 180)) for the azimuth, in degrees, km or km/s for the others.  The bound is the measured figure x 8
rounded up to one significant digit - the run is deterministic, the margin covers a compiler or libm change of a few ulp - and
never above the ceilings 1e-9 deg / 1e-9 km (km/s): a deviation above the ceiling is a bug, not a tolerance.  A measured 0 stays
0; `Visible` is always exact.  The hand-placed states (every parameter equal to the host definition to the last bit there), the
windows and the Monte Carlo (tests 2, 4, 8) measure no more than these figures and use this table.  The stations of that run stood
around (22.1467, 249.1561) deg: 7 visible samples per run and station, smallest horizontal range 49.54 km, nearest |elevation - mask|
1.40 deg (A) / 0.025 deg (B), azimuths from B at sample 20 from 0.000 to 359.973 deg.

    parameter            measured    unit   bound
    Azimuth              5.684e-14   deg    5e-13
    Elevation            1.599e-14   deg    2e-13
    Range                9.095e-13   km     8e-12
    RangeRate            2.665e-15   km/s   3e-14
    ElevationAboveMask   2.842e-14   deg    3e-13
    Visible              0           -      0
    RhoS                 4.547e-13   km     4e-12
    RhoE                 9.095e-13   km     8e-12
    RhoZ                 1.137e-12   km     1e-11
"""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import nyx_amd as nx
from nyx_amd import _abi, ephem
from nyx_amd.groundtrack import GroundTrackParameter as G, ground_track_value
from nyx_amd.stations import AerParameter as A, aer_value, station_consts
from scenarios import EPOCH0_NS, dispersed_leo_batch, leo_full_setup, leo_nominal

pytestmark = pytest.mark.gpu

S = nx.NS_PER_S
STEP = 60 * S
DUR = 5400 * S
COUNT = 91
K_PASS = 20        # the sample of run 0 the stations are placed around
A_KM, F = 6378.1363, 1.0 / 298.257
IAU_EARTH = nx.Frame(nx.EARTH, ephem.MU_EARTH, A_KM, nx.IAU_EARTH_ROTATION, F)
INERTIAL = nx.Frame(nx.EARTH, ephem.MU_EARTH, A_KM, None, F)
ALL = list(A)
CEILING = 1e-9     # deg, km or km/s
# parameter -> bound: see the table above
TOL = {
    A.Azimuth: 5e-13,
    A.Elevation: 2e-13,
    A.Range: 8e-12,
    A.RangeRate: 3e-14,
    A.ElevationAboveMask: 3e-13,
    A.Visible: 0.0,
    A.RhoS: 4e-12,
    A.RhoE: 8e-12,
    A.RhoZ: 1e-11,
}


def deviation(p, got, want):
    """Largest difference of one parameter over the samples: wrapped degrees for the azimuth, absolute for the others."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and np.isfinite(want).all() and np.isfinite(got).all(), p.name
    if not got.size:
        return 0.0
    if p is A.Azimuth:
        return float(np.abs((got - want + 180.0) % 360.0 - 180.0).max())
    return float(np.abs(got - want).max())


def assert_all_within(params, got, want, label=""):
    """got / want [S, P, ...]: every parameter over all stations and samples inside its bound."""
    failures = []
    for j, p in enumerate(params):
        d = deviation(p, got[:, j], want[:, j])
        print(f"deviation{label} {p.name:18s} {d:.3e}  (bound {TOL[p]:.0e})")
        assert TOL[p] <= CEILING
        if not d <= TOL[p]:
            failures.append(f"{p.name}: {d:.3e} > {TOL[p]:.0e}")
    assert not failures, "\n".join(failures)


def host_values(stations, params, rv, epochs):
    """[S, P, ...] of the host definition."""
    return np.stack([np.stack([aer_value(p, rv, epochs, st) for p in params]) for st in stations])


@pytest.fixture(scope="module")
def leo():
    prop, almanac, central = leo_full_setup(degree=8)
    compiled = prop.compile(almanac, central)
    ctx = nx.GpuContext(compiled)
    yield prop, almanac, central, compiled, ctx
    ctx.close()


@pytest.fixture(scope="module")
def leo70(leo):
    """One orbit of 70 dispersed trajectories with dense output, its traj_every states, the two stations and the host definition
    on those states: computed once, shared, never written to."""
    ctx = leo[4]
    _, st, traj = ctx.propagate_with_traj(dispersed_leo_batch(70, seed=11), DUR, capacity=256)
    assert (st.status == 0).all()
    ev = ctx.traj_every(traj, STEP, COUNT)
    assert (ev.len == COUNT).all()
    rv = np.ascontiguousarray(ev.state.transpose(1, 2, 0))             # [K, n, 6]
    lat, lon = (float(ground_track_value(p, rv[K_PASS, 0], ev.epoch_ns[K_PASS, 0], IAU_EARTH)) for p in (G.Latitude, G.Longitude))
    assert abs(lat) < 89.0
    stations = [nx.GroundStation("A", lat + 0.5, lon, 0.5, IAU_EARTH, 5.0), nx.GroundStation("B", lat - 0.5, lon, 0.5, IAU_EARTH, 5.0)]
    want = host_values(stations, ALL, rv, ev.epoch_ns)                  # [2, 9, K, n]
    # what lets the comparisons leave out no sample
    vis = want[:, ALL.index(A.Visible)]
    horizontal = np.sqrt(want[:, ALL.index(A.RhoS)] ** 2 + want[:, ALL.index(A.RhoE)] ** 2)
    on_mask = np.abs(want[:, ALL.index(A.ElevationAboveMask)])
    print(f"stations around ({lat:.4f}, {lon:.4f}): visible samples per run {vis.sum(axis=1).min(axis=1)} .. {vis.sum(axis=1).max(axis=1)}, "
          f"smallest horizontal range {horizontal.min():.2f} km, nearest |elevation - mask| {on_mask.min(axis=(1, 2))} deg, "
          f"azimuth from B at sample {K_PASS}: {want[1, 0, K_PASS].min():.3f} .. {want[1, 0, K_PASS].max():.3f}")
    assert np.isfinite(want).all()
    assert ((vis == 1.0).any(axis=1) & (vis == 0.0).any(axis=1)).all()          # every run is seen and lost by either station
    assert horizontal.min() > 1.0 and on_mask.min() > 1e-6
    for a in (ev.state, ev.epoch_ns, rv, want):
        a.setflags(write=False)
    return traj, ev, rv, want, stations


def head(traj, n):
    """The first n trajectories of a batch as a batch of their own."""
    t = _abi.TrajBatch(n, traj.capacity)
    t.epoch_ns[:], t.state[:], t.len[:] = traj.epoch_ns[:, :n], traj.state[:, :, :n], traj.len[:n]
    return t


def head_one(traj, i):
    t = _abi.TrajBatch(1, traj.capacity)
    t.epoch_ns[:, 0], t.state[:, :, 0], t.len[0] = traj.epoch_ns[:, i], traj.state[:, :, i], traj.len[i]
    return t


def aer_query(stations, params, step=STEP, start=None, stop=None):
    q = _abi.AerQuery()
    q.n_params, q.step_ns, q.n_stations = len(params), step, len(stations)
    for k, p in enumerate(params):
        q.param[k] = _abi.AER_PARAM[p.name]
    if start is not None:
        q.has_window, q.start_ns, q.end_ns = 1, start, stop
    nx.fill_gt_frame(q, stations[0].frame)
    for k, st in enumerate(stations):
        q.stations[k].latitude_deg, q.stations[k].longitude_deg = st.latitude_deg, st.longitude_deg
        q.stations[k].height_km, q.stations[k].elevation_mask_deg = st.height_km, st.elevation_mask_deg
    return q


@pytest.mark.parametrize("n", [1, 64, 65, 70])
def test_1_all_parameters_against_the_host_definition(leo, leo70, n):
    ctx = leo[4]
    traj, want, stations = head(leo70[0], n), leo70[3], leo70[4]
    assert set(TOL) == set(ALL)
    for cap in (15, 16, 17, 91, 100):                                          # chunk seams at 16
        vals, length = ctx.traj_aer(traj, stations, ALL, STEP, capacity=cap)    # nine parameters: two launches
        assert vals.shape == (2, 9, cap, n) and length.dtype == np.int32 and (length == COUNT).all()
        m = min(COUNT, cap)
        assert np.isnan(vals[:, :, m:]).all()                                   # the kernel blanks what it did not produce
        assert_all_within(ALL, vals[:, :, :m], want[:, :, :m, :n], label=f" n={n} cap={cap}")
        np.testing.assert_array_equal(vals[:, ALL.index(A.Visible), :m], want[:, ALL.index(A.Visible), :m, :n])
    az = vals[:, 0, :m]
    assert (az >= 0.0).all() and (az < 360.0).all()
    v2, l2 = ctx.traj_aer(traj, stations, ALL, STEP)                            # capacity=None: sized from the batch's epochs
    assert v2.shape == (2, 9, COUNT, n)
    np.testing.assert_array_equal(v2, vals[:, :, :COUNT])
    if n == 70:   # the azimuths seen from B at the pass straddle the 0 / 360 wrap: compared wrapped, stored in [0, 360)
        at_pass = vals[1, 0, K_PASS]
        assert at_pass.min() < 90.0 and at_pass.max() > 270.0


def test_2_hand_placed_states_without_a_rotation(leo):
    """has_frame = 0 and stored epochs = sample epochs: traj_at returns the stored states, the frame is the identity, so the
    hand-placed geometry reaches the station block exactly as placed."""
    ctx = leo[4]
    st = nx.GroundStation("hand", 35.247164, -116.795, 1.07114904, INERTIAL, 5.0)
    c = station_consts(st)
    r, sv, ev_, zv = (np.asarray(v) for v in (c.r_km, c.south, c.east, c.zenith))
    places = np.stack([r + 400.0 * zv, r + 100.0 * ev_, r - 100.0 * ev_, r - 100.0 * sv, r + 100.0 * sv, r])   # zenith, E, W, N, S, the station
    ZENITH, STATION = 0, 5
    n, k_n = len(places), 5
    t = _abi.TrajBatch(n, k_n)
    t.len[:] = k_n
    t.epoch_ns[:] = (EPOCH0_NS + STEP * np.arange(k_n))[:, None]
    for k in range(k_n):
        t.state[:3, k, :] = places.T
        t.state[3:, k, :] = np.array([0.3, -7.0, 1.0])[:, None]
    vals, length = ctx.traj_aer(t, [st], ALL, STEP)
    assert vals.shape == (1, 9, k_n, n) and (length == k_n).all()               # the sample AT the station is counted
    rv = np.ascontiguousarray(t.state.transpose(1, 2, 0))
    want = host_values([st], ALL, rv, t.epoch_ns)
    idx = np.arange(n)
    for j, p in enumerate(ALL):
        if p is A.Azimuth:
            cols = (idx != ZENITH) & (idx != STATION)                           # no azimuth at the zenith or at the station
        elif p in (A.Elevation, A.ElevationAboveMask, A.RangeRate):
            cols = idx != STATION                                                # no direction at the station: NaN, checked below
        else:
            cols = idx >= 0                                                      # Range, Rho*, Visible: finite everywhere
        d = deviation(p, vals[0, j][:, cols], want[0, j][:, cols])
        print(f"deviation hand-placed {p.name:18s} {d:.3e}  (bound {TOL[p]:.0e})")
        assert d <= TOL[p], f"{p.name}: {d:.3e} > {TOL[p]:.0e}"
    get = lambda p: vals[0, ALL.index(p)]
    # the absolute figures of the host test (tests/test_aer_host.py): 1e-9 deg, 1e-9 km
    assert np.abs(get(A.Range)[:, ZENITH] - 400.0).max() <= 1e-9 and np.abs(get(A.Elevation)[:, ZENITH] - 90.0).max() <= 1e-9
    for col, azimuth in ((1, 90.0), (2, 270.0), (3, 0.0), (4, 180.0)):
        az = get(A.Azimuth)[:, col]
        assert (az >= 0.0).all() and (az < 360.0).all()
        assert np.abs((az - azimuth + 180.0) % 360.0 - 180.0).max() <= 1e-9, (col, az)
        assert np.abs(get(A.Elevation)[:, col]).max() <= 1e-9 and np.abs(get(A.Range)[:, col] - 100.0).max() <= 1e-9
        assert (get(A.Visible)[:, col] == 0.0).all()                             # on the horizon, under a mask of 5 deg
    assert (get(A.Visible)[:, ZENITH] == 1.0).all()
    # AT the station: range 0, no direction - NaN on both sides -, not visible
    assert (get(A.Range)[:, STATION] == 0.0).all() and (want[0, ALL.index(A.Range)][:, STATION] == 0.0).all()
    for p in (A.Elevation, A.ElevationAboveMask, A.RangeRate):
        assert np.isnan(get(p)[:, STATION]).all() and np.isnan(want[0, ALL.index(p)][:, STATION]).all(), p.name
    assert (get(A.Visible)[:, STATION] == 0.0).all() and (want[0, ALL.index(A.Visible)][:, STATION] == 0.0).all()


def grid_stations(leo70):
    """A, B and a 14-point grid: both poles, negative longitudes, the date line."""
    grid = [(90.0, 0.0), (-90.0, 123.4), (0.0, 0.0), (0.0, 180.0), (0.0, -90.0), (45.0, -116.795), (-45.0, 148.98), (60.0, 4.25),
            (-60.0, -70.6), (30.0, 359.9), (-30.0, 243.205), (75.0, -179.9), (-75.0, 90.0), (10.0, 725.0)]
    return list(leo70[4]) + [nx.GroundStation(f"g{k}", la, lo, 0.1 * k, IAU_EARTH, float(k)) for k, (la, lo) in enumerate(grid)]


def test_3_sixteen_stations_in_one_launch_and_the_splits(leo, leo70):
    ctx = leo[4]
    traj = leo70[0]
    sixteen = grid_stations(leo70)
    assert len(sixteen) == 16
    params = [A.Azimuth, A.Elevation, A.Range, A.RangeRate, A.Visible]
    together, ln = ctx.traj_aer(traj, sixteen, params, STEP, capacity=COUNT)
    assert together.shape == (16, 5, COUNT, traj.n) and np.isfinite(together).all()
    for s, st in enumerate(sixteen):
        alone, l1 = ctx.traj_aer(traj, [st], params, STEP, capacity=COUNT)
        np.testing.assert_array_equal(alone[0], together[s], err_msg=st.name)    # bit for bit
        np.testing.assert_array_equal(l1, ln)
    seventeen = sixteen + [nx.GroundStation("extra", 12.0, 34.0, 0.0, IAU_EARTH, 0.0)]
    split, l17 = ctx.traj_aer(traj, seventeen, params, STEP, capacity=COUNT)    # 16 + 1: two launches
    assert split.shape == (17, 5, COUNT, traj.n)
    np.testing.assert_array_equal(split[:16], together)
    np.testing.assert_array_equal(split[16], ctx.traj_aer(traj, seventeen[16:], params, STEP, capacity=COUNT)[0][0])
    np.testing.assert_array_equal(l17, ln)
    # eight parameters together = eight alone; nine = 8 + 1
    eight = ALL[:8]
    both = sixteen[:2]
    t8, l8 = ctx.traj_aer(traj, both, eight, STEP, capacity=COUNT)
    for j, p in enumerate(eight):
        alone, l1 = ctx.traj_aer(traj, both, [p], STEP, capacity=COUNT)
        np.testing.assert_array_equal(alone[:, 0], t8[:, j], err_msg=p.name)
        np.testing.assert_array_equal(l1, l8)
    t9, l9 = ctx.traj_aer(traj, both, ALL, STEP, capacity=COUNT)
    assert t9.shape == (2, 9, COUNT, traj.n)
    np.testing.assert_array_equal(t9[:, :8], t8)
    np.testing.assert_array_equal(t9[:, 8], ctx.traj_aer(traj, both, [ALL[8]], STEP, capacity=COUNT)[0][:, 0])
    np.testing.assert_array_equal(l9, l8)
    with pytest.raises(TypeError):
        ctx.traj_aer(traj, both, [A.Range, G.Rmag], STEP)


def host_series(ctx, traj, stations, params, start=None, stop=None, step=STEP):
    """The host composition per run: (values[S, P, K, n] NaN-padded, len[n], first[n]) from traj_at + aer_value."""
    lo, hi = nx.series_bounds(traj, start, stop)
    counts = np.where(hi >= lo, (hi - lo) // step + 1, 0)
    k_max = int(counts.max()) if len(counts) else 0
    out = np.full((len(stations), len(params), k_max, traj.n), np.nan)
    for i in range(traj.n):
        if counts[i] == 0:
            continue
        q = int(lo[i]) + step * np.arange(int(counts[i]), dtype=np.int64)
        states, status = ctx.traj_at(head_one(traj, i), q)
        assert not _abi.interp_failed(status).any()
        out[:, :, :counts[i], i] = host_values(stations, params, states[:, 0], q)
    return out, counts.astype(np.int32), lo


def test_4_windows_against_the_host_composition(leo, leo70):
    ctx = leo[4]
    traj, stations = head(leo70[0], 65), leo70[4]
    end = EPOCH0_NS + DUR
    params = [A.Azimuth, A.Elevation, A.Range, A.RangeRate, A.Visible]
    windows = [(EPOCH0_NS + 777 * S, EPOCH0_NS + 3000 * S + 5, 38),      # clips both ends
               (EPOCH0_NS - 1000 * S, EPOCH0_NS + 2000 * S, 34),          # clips the end only (the start is clamped to the first epoch)
               (EPOCH0_NS - STEP, end + STEP, 91),                        # clips nothing
               (end + S, end + 100 * S, 0)]                               # empty: after the runs
    for start, stop, count in windows:
        vals, length = ctx.traj_aer(traj, stations, params, STEP, start, stop)
        want, want_len, first = host_series(ctx, traj, stations, params, start, stop)
        np.testing.assert_array_equal(length, want_len)
        assert (length == count).all() and vals.shape == (2, 5, max(count, 1), 65)
        if count:
            assert (first == max(start, EPOCH0_NS)).all()
            assert_all_within(params, vals, want, label=f" window {count}")
        else:
            assert np.isnan(vals).all()


def test_5_capacity_below_the_produced_count(leo, leo70):
    ctx = leo[4]
    lib = _abi.load_library()
    traj, stations = leo70[0], leo70[4]
    n, cap, guard = traj.n, 50, 1000
    params = [A.Elevation, A.Range, A.Visible]
    full, _ = ctx.traj_aer(traj, stations, params, STEP, capacity=COUNT)
    size = 2 * 3 * cap * n
    buf = np.full(size + guard, 12345.0)
    length = np.full(n + 8, -7, dtype=np.int32)
    q = aer_query(stations, params)
    cin = traj.as_c()
    rc = lib.nyx_hip_traj_aer(ctx._h, C.byref(cin), n, C.byref(q), cap, buf.ctypes.data_as(_abi.c_double_p), length.ctypes.data_as(_abi.c_int32_p))
    assert rc == 0, _abi.last_error()
    assert (length[:n] == COUNT).all() and (length[n:] == -7).all()          # produced, not stored
    np.testing.assert_array_equal(buf[:size].reshape(2, 3, cap, n), full[:, :, :cap])
    assert (buf[size:] == 12345.0).all()                                      # nothing beyond n_stations * n_params * capacity * n


def test_6_device_pointers_on_a_stream_equal_the_host_flavour(leo, leo70):
    import torch
    ctx = leo[4]
    lib = _abi.load_library()
    dev = torch.device("cuda", 0)
    t, stations = leo70[0], leo70[4]
    n, cap, guard = t.n, 40, 512
    params = [A.Azimuth, A.Elevation, A.RangeRate]
    start, stop = EPOCH0_NS + 500 * S, EPOCH0_NS + 5000 * S
    host, host_len = ctx.traj_aer(t, stations, params, STEP, start, stop, capacity=cap)
    epoch = torch.from_numpy(t.epoch_ns).to(dev)
    state = torch.from_numpy(t.state).to(dev)
    tlen = torch.from_numpy(t.len).to(dev)
    s = _abi.Traj()
    s.capacity = t.capacity
    s.epoch_ns = C.cast(epoch.data_ptr(), _abi.c_int64_p)
    for k, f in enumerate(["x_km", "y_km", "z_km", "vx_km_s", "vy_km_s", "vz_km_s"]):
        setattr(s, f, C.cast(state[k].data_ptr(), _abi.c_double_p))
    s.len = C.cast(tlen.data_ptr(), _abi.c_int32_p)
    size = 2 * 3 * cap * n
    values = torch.full((size + guard,), 12345.0, dtype=torch.float64, device=dev)
    length = torch.full((n + 8,), -7, dtype=torch.int32, device=dev)
    q = aer_query(stations, params, start=start, stop=stop)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        rc = lib.nyx_hip_traj_aer_device(ctx._h, C.byref(s), n, C.byref(q), cap, C.c_void_p(values.data_ptr()), C.c_void_p(length.data_ptr()),
                                         C.c_void_p(stream.cuda_stream))
    assert rc == 0, _abi.last_error()
    stream.synchronize()
    got, got_len = values.cpu().numpy(), length.cpu().numpy()
    np.testing.assert_array_equal(got_len[:n], host_len)
    assert (got_len[n:] == -7).all() and (host_len == 76).all()                # (5000 - 500) / 60 + 1 produced, 40 stored
    np.testing.assert_array_equal(got[:size].reshape(2, 3, cap, n), host)
    assert (got[size:] == 12345.0).all()                                        # guard values: nothing beyond the buffer


def test_7_the_series_ends_at_the_first_sample_that_cannot_be_interpolated(leo, leo70):
    """Two stored states 10 ns apart are the same f64 second: InterpMath for every window that holds them.  The series of that
    trajectory ends there (traj_it.rs:39-61), as nyx_hip_traj_every reports, and what later chunks could interpolate again is
    blanked for EVERY station (the trajectory of test 10 of tests/test_gpu_groundtrack.py)."""
    ctx = leo[4]
    stations = leo70[4]
    rng = np.random.default_rng(9)
    t = _abi.TrajBatch(2, 20)
    t.len[:] = 20
    for i in range(2):
        t.epoch_ns[:, i] = EPOCH0_NS + i * 13 + np.cumsum(rng.integers(5, 120, size=20)) * 10**9 + rng.integers(0, 10**9, size=20)
    t.state[:] = rng.standard_normal(t.state.shape) * 7000.0
    t.epoch_ns[8, 1] = t.epoch_ns[7, 1] + 10
    ev = ctx.traj_every(t, 10**9, 4096)
    vals, length = ctx.traj_aer(t, stations, [A.Range, A.Elevation, A.Visible], 10**9, capacity=4096)
    np.testing.assert_array_equal(length, ev.len)
    assert 0 < length[1] < length[0]             # trajectory 1 ends early: its first windows hold the coincident pair
    for i in range(2):
        m = int(length[i])
        assert np.isfinite(vals[:, :, :m, i]).all() and np.isnan(vals[:, :, m:, i]).all()
    first1 = int(t.epoch_ns[0, 1])
    k_late = int((t.epoch_ns[17, 1] - first1) // 10**9) + 1
    at, status = ctx.traj_at(t, [first1 + k_late * 10**9])
    assert status[0, 1] == _abi.INTERP_OK and np.isfinite(at[0, 1]).all() and k_late > 16 + length[1]
    assert np.isnan(vals[:, :, k_late, 1]).all()


def test_8_results_station_views_on_a_real_monte_carlo(leo, leo70):
    prop, almanac, central = leo[:3]
    stations = leo70[4]
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
    views = res.station_views(stations, STEP, ALL)
    ctx = res._traj_ctx
    assert hasattr(ctx, "traj_aer")

    class Compose:   # the evaluator of the definition: traj_every / traj_at only
        traj_at = staticmethod(ctx.traj_at)
        traj_every = staticmethod(ctx.traj_every)

    want = dataclasses.replace(res, _traj_ctx=Compose).station_views(stations, STEP, ALL)
    assert isinstance(views, nx.AerSeries) and views.values.shape == want.values.shape == (2, 9, COUNT, 70)
    np.testing.assert_array_equal(views.len, want.len)
    np.testing.assert_array_equal(views.epoch0_ns, want.epoch0_ns)
    np.testing.assert_array_equal(views.ok, want.ok)
    assert views.len[fail] == 0 and np.isnan(views.values[:, :, :, fail]).all() and list(np.delete(views.len, fail)) == [COUNT] * 69
    assert list(views.epochs(0)) == [EPOCH0_NS + k * STEP for k in range(COUNT)] and len(views.epochs(fail)) == 0
    okc = np.nonzero(views.ok)[0]
    on_mask = np.abs(want.values[:, ALL.index(A.ElevationAboveMask)][:, :, okc]).min()
    print(f"monte carlo: nearest |elevation - mask| {on_mask:.3e} deg")
    assert on_mask > 1e-6                                                       # (no sample of THIS ensemble on the mask either)
    assert_all_within(ALL, views.values[:, :, :, okc], want.values[:, :, :, okc], label=" mc")
    np.testing.assert_array_equal(views.values[:, ALL.index(A.Visible)][:, :, okc], want.values[:, ALL.index(A.Visible)][:, :, okc])
    # one trajectory through Traj.station_view: the default set is what a one-way measurement reads
    ep, one = res.runs[0].result.traj.station_view(stations, STEP)
    assert list(ep) == [EPOCH0_NS + k * STEP for k in range(COUNT)] and one.shape == (2, 4, COUNT)
    np.testing.assert_array_equal(one, views.values[:, :4, :, 0])
    # the whole ensemble passes over A at the sample the stations were placed around, and is on the far side 40 minutes later
    frac = views.visible_fraction(stations[0])
    assert frac.shape == (COUNT,) and frac[K_PASS] == 1.0 and frac[60] == 0.0
    np.testing.assert_array_equal(frac, want.visible_fraction(0))
