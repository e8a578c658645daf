"""CPU: the host definition of the station views (nyx_amd/stations.py) against itself and against geometry - no GPU, no kernel.

The definition is a RESTATEMENT of the published formulas (anise's `azimuth_elevation_range_sez` is not part of the reference tree):
what pins it here is geometry that does not depend on it.

* a state on the station's zenith line, H above it, is seen at range H and elevation 90; states 100 km along +-E^ / -+S^ at
  azimuth 90 / 270 / 0 / 180 and elevation 0 (measured at 1e-13 deg and km; held to 1e-9);
* FRAME INVARIANCE: range and range rate are the same computed in the inertial frame, where the station sits at R^T r_st and moves
  with (w pole) x R^T r_st, the pole being row 3 of `iau_dcm` (measured 3.6e-12 km and 2.2e-15 km/s on a two-body orbit; held to
  1e-10 km and 1e-12 km/s);
* CONSISTENCY WITH THE GROUND TRACK: a station at the ground-track latitude / longitude of a state, at height 0, has the state at
  its zenith at a range equal to the ground-track Height (1e-6 km: the geodetic iteration stops at 1e-12 rad);
* `Results.station_views` by composition (the injected oracle evaluator of tests/test_groundtrack_host.py: no fused entry) gives
  the same `len` / `epoch0_ns` / `ok` as `Results.ground_tracks`, and the values of `aer_value` on the resampled states."""
import math

import numpy as np
import pytest

import nyx_amd as nx
import oracle_lib
from nyx_amd import _abi, ephem, groundtrack as gt, stations as stn
from nyx_amd.groundtrack import GroundTrackParameter as G
from nyx_amd.stations import AerParameter as A
from scenarios import EPOCH0_NS, leo_full_setup, leo_nominal

S = nx.NS_PER_S
STEP = 60 * S
A_KM, F = 6378.1363, 1.0 / 298.257
IAU_EARTH = nx.Frame(nx.EARTH, ephem.MU_EARTH, A_KM, nx.IAU_EARTH_ROTATION, F)
MADRID = nx.GroundStation("Madrid", 40.427222, 4.250556, 0.834939, IAU_EARTH, 5.0)
CANBERRA = nx.GroundStation("Canberra", -35.398333, 148.981944, 0.691750, IAU_EARTH, 5.0)
ALL = list(A)
FAILED = 3


def _fixed(station, along, km):
    """[6]: a body-fixed state `km` from the station along the unit vector `along`, at rest in the frame."""
    c = stn.station_consts(station)
    return np.concatenate([np.asarray(c.r_km) + km * np.asarray(along), np.zeros(3)])


@pytest.mark.parametrize("station", [MADRID, CANBERRA, nx.GroundStation("pole", 90.0, 0.0, 0.0, IAU_EARTH), nx.GroundStation("eq", 0.0, -70.0, 2.0, IAU_EARTH)])
def test_zenith_and_the_four_horizontal_directions(station):
    c = stn.station_consts(station)
    val = lambda p, y: float(stn.sez_value(p, y, c))
    up = _fixed(station, c.zenith, 400.0)
    assert abs(val(A.Range, up) - 400.0) <= 1e-9 and abs(val(A.Elevation, up) - 90.0) <= 1e-9     # (the azimuth is undefined there)
    assert abs(val(A.RhoZ, up) - 400.0) <= 1e-9 and abs(val(A.RhoS, up)) <= 1e-9 and abs(val(A.RhoE, up)) <= 1e-9
    neg = lambda v: tuple(-x for x in v)
    for along, azimuth in ((c.east, 90.0), (neg(c.east), 270.0), (neg(c.south), 0.0), (c.south, 180.0)):
        y = _fixed(station, along, 100.0)
        az = val(A.Azimuth, y)
        assert 0.0 <= az < 360.0
        assert abs((az - azimuth + 180.0) % 360.0 - 180.0) <= 1e-9, (station.name, azimuth, az)      # (north: 0, wrapped)
        assert abs(val(A.Elevation, y)) <= 1e-9 and abs(val(A.Range, y) - 100.0) <= 1e-9
        assert val(A.RangeRate, y) == 0.0
        assert val(A.ElevationAboveMask, y) == val(A.Elevation, y) - station.elevation_mask_deg
    # the triad is right-handed and orthonormal, the zenith the ellipsoid's normal
    assert np.abs(np.cross(c.south, c.east) - np.asarray(c.zenith)).max() <= 1e-15
    lat, h = gt.geodetic(np.asarray(c.r_km), A_KM, F)
    assert abs(float(lat) - station.latitude_deg) <= 1e-9 and abs(float(h) - station.height_km) <= 1e-6


def test_the_wrap_the_mask_and_the_station_itself():
    st = nx.GroundStation("s", 10.0, 20.0, 0.0, IAU_EARTH, 5.0)
    c = stn.station_consts(st)
    # due north with a west component of 1e-17 of the range (an axis-aligned triad at the origin makes the components exact): a
    # negative angle that + 360 would round to 360 is 0
    axes = stn.StationConsts((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), 0.0)
    assert float(stn.sez_value(A.Azimuth, [-1.0, -1e-17, 0.0, 0.0, 0.0, 0.0], axes)) == 0.0
    assert float(stn.sez_value(A.Azimuth, [-1.0, -0.0, 0.0, 0.0, 0.0, 0.0], axes)) == 0.0
    assert abs(float(stn.sez_value(A.Azimuth, [-1.0, -1e-9, 0.0, 0.0, 0.0, 0.0], axes)) - (360.0 - 1e-9 * 180.0 / math.pi)) <= 1e-13
    assert float(stn.sez_value(A.Azimuth, [1.0, 0.0, 0.0, 0.0, 0.0, 0.0], axes)) == 180.0
    # the mask: Visible is elevation - mask >= 0
    for el, seen in ((4.0, 0.0), (6.0, 1.0), (90.0, 1.0), (-20.0, 0.0)):
        along = tuple(-math.cos(math.radians(el)) * s + math.sin(math.radians(el)) * z for s, z in zip(c.south, c.zenith))
        y = _fixed(st, along, 700.0)
        assert abs(float(stn.sez_value(A.Elevation, y, c)) - el) <= 1e-9
        assert float(stn.sez_value(A.Visible, y, c)) == seen
        assert float(stn.sez_value(A.ElevationAboveMask, y, c)) == float(stn.sez_value(A.Elevation, y, c)) - 5.0
    # AT the station: range 0, no direction - elevation and range rate NaN, not visible
    here = _fixed(st, c.zenith, 0.0)
    assert float(stn.sez_value(A.Range, here, c)) == 0.0
    assert math.isnan(float(stn.sez_value(A.Elevation, here, c))) and math.isnan(float(stn.sez_value(A.RangeRate, here, c)))
    assert math.isnan(float(stn.sez_value(A.ElevationAboveMask, here, c))) and float(stn.sez_value(A.Visible, here, c)) == 0.0
    with pytest.raises(TypeError):
        stn.sez_value(G.Latitude, here, c)


def _two_body_orbit():
    """[91, 6] at 60 s: the LEO nominal under two-body gravity (RK4, 1 s) - a stand-in, only its smoothness matters here."""
    mu = ephem.MU_EARTH
    y = leo_nominal().astype(np.float64).copy()

    def f(y):
        r = y[:3]
        return np.concatenate([y[3:], -mu * r / np.linalg.norm(r) ** 3])

    out = [y.copy()]
    for s in range(5400):
        k1 = f(y); k2 = f(y + 0.5 * k1); k3 = f(y + 0.5 * k2); k4 = f(y + k3)   # noqa: E702
        y = y + (k1 + 2 * k2 + 2 * k3 + k4) / 6.0
        if (s + 1) % 60 == 0:
            out.append(y.copy())
    return np.stack(out)


def test_range_and_range_rate_do_not_depend_on_the_frame():
    rv = _two_body_orbit()
    ep = EPOCH0_NS + STEP * np.arange(len(rv), dtype=np.int64)
    m, wdot = gt.iau_dcm(nx.IAU_EARTH_ROTATION, ep)
    for st in (MADRID, CANBERRA):
        r_st = np.asarray(stn.station_consts(st).r_km)
        r_in = np.einsum("kji,j->ki", m, r_st)                          # R^T r_st
        v_in = np.cross(wdot[:, None] * m[:, 2, :], r_in)                # (w pole) x R^T r_st
        rho, rho_dot = rv[:, :3] - r_in, rv[:, 3:] - v_in
        rng = np.linalg.norm(rho, axis=1)
        d_range = np.abs(rng - stn.aer_value(A.Range, rv, ep, st)).max()
        d_rate = np.abs((rho * rho_dot).sum(axis=1) / rng - stn.aer_value(A.RangeRate, rv, ep, st)).max()
        print(f"{st.name}: inertial against body-fixed: range {d_range:.3e} km, range rate {d_rate:.3e} km/s")
        assert d_range <= 1e-10 and d_rate <= 1e-12
        assert np.abs(stn.aer_value(A.RangeRate, rv, ep, st)).max() > 1.0   # (a pass and the far side: km/s)


def test_a_station_under_the_ground_track_sees_the_state_at_its_zenith():
    rv = _two_body_orbit()[::9]
    ep = EPOCH0_NS + 9 * STEP * np.arange(len(rv), dtype=np.int64)
    lat, lon, height = (gt.ground_track_value(p, rv, ep, IAU_EARTH) for p in (G.Latitude, G.Longitude, G.Height))
    for k in range(len(rv)):
        st = nx.GroundStation("under", float(lat[k]), float(lon[k]), 0.0, IAU_EARTH)
        rng, el = float(stn.aer_value(A.Range, rv[k], ep[k], st)), float(stn.aer_value(A.Elevation, rv[k], ep[k], st))
        assert abs(rng - float(height[k])) <= 1e-6 and el > 89.999, (k, rng, float(height[k]), el)
        assert float(stn.aer_value(A.Visible, rv[k], ep[k], st)) == 1.0


def test_aer_value_composes_to_body_fixed_and_the_constants_and_broadcasts():
    rv = _two_body_orbit()[:12].reshape(3, 4, 6)
    ep = (EPOCH0_NS + STEP * np.arange(12, dtype=np.int64)).reshape(3, 4)
    yf = gt.to_body_fixed(rv, ep, IAU_EARTH)
    c = stn.station_consts(MADRID)
    for p in ALL:
        got = stn.aer_value(p, rv, ep, MADRID)
        assert got.shape == (3, 4) and got.dtype == np.float64
        np.testing.assert_array_equal(got, stn.sez_value(p, yf, c))
        np.testing.assert_array_equal(got[1, 2], stn.aer_value(p, rv[1, 2], ep[1, 2], MADRID))
    rho = np.stack([stn.aer_value(p, rv, ep, MADRID) for p in (A.RhoS, A.RhoE, A.RhoZ)])
    np.testing.assert_array_equal(stn.aer_value(A.Range, rv, ep, MADRID), np.sqrt(rho[0] * rho[0] + rho[1] * rho[1] + rho[2] * rho[2]))
    assert stn.DEFAULT_PARAMS == (A.Azimuth, A.Elevation, A.Range, A.RangeRate)
    with pytest.raises(ValueError, match="latitude"):
        stn.aer_value(A.Range, rv, ep, nx.GroundStation("bad", 91.0, 0.0, 0.0, IAU_EARTH))


class OracleTraj:
    """What Results needs from a context: traj_at / traj_every (GpuContext's signatures); no traj_aer."""

    traj_at = staticmethod(oracle_lib.traj_at)
    traj_every = staticmethod(oracle_lib.traj_every)


def test_results_station_views_by_composition():
    """Five runs, one failed, four samples: the gather of the ground tracks, the values of the definition."""
    prop, almanac, central = leo_full_setup(degree=4)
    compiled = prop.compile(almanac, central)
    template = nx.Spacecraft(EPOCH0_NS, leo_nominal(), central, dry_mass_kg=100.0, prop_mass_kg=10.0, srp_area_m2=1.0, cr=1.8)
    mvn = nx.MvnSpacecraft.from_sigmas(template, [1.0, 1.0, 1.0, 1e-3, 1e-3, 1e-3])

    def fn(batch, end_epoch_ns):
        out, st, traj = oracle_lib.propagate_with_traj(compiled, batch, end_epoch_ns - int(batch.epoch_ns[0]), 256)
        st.status[FAILED] = nx._abi.ERR_NAN
        return out, st, traj, OracleTraj

    res = nx.MonteCarlo(mvn, seed=3, propagate_fn=fn).run_until_epoch(prop, almanac, EPOCH0_NS + 3 * STEP, 5)
    assert isinstance(res.runs[FAILED].result, nx.PropagationError)
    # a station under the first sample of run 0 (it sees the ensemble) and one on the far side (it does not)
    tb = res._traj_batch
    row0 = res._traj_rows[res.runs[0].index]
    first = tb.state[:, 0, row0]
    lat, lon = (float(gt.ground_track_value(p, first, EPOCH0_NS, IAU_EARTH)) for p in (G.Latitude, G.Longitude))
    near = nx.GroundStation("near", lat, lon, 0.2, IAU_EARTH, 5.0)
    far = nx.GroundStation("far", -lat, (lon + 180.0) % 360.0, 0.2, IAU_EARTH, 5.0)
    views = res.station_views([near, far], STEP, ALL)
    gs = res.ground_tracks(IAU_EARTH, STEP, [G.Latitude])
    assert isinstance(views, nx.AerSeries) and views.values.shape == (2, 9, 4, 5) and views.step_ns == STEP
    assert views.stations == [near, far] and views.params == ALL
    for name in ("len", "epoch0_ns", "ok"):
        assert getattr(views, name).dtype == getattr(gs, name).dtype
        np.testing.assert_array_equal(getattr(views, name), getattr(gs, name))
    assert list(views.len) == [0 if j == FAILED else 4 for j in range(5)] and list(views.epochs(1)) == [EPOCH0_NS + k * STEP for k in range(4)]
    assert np.isnan(views.values[:, :, :, FAILED]).all() and len(views.epochs(FAILED)) == 0
    ev = oracle_lib.traj_every(tb, STEP, 4)
    q = EPOCH0_NS + STEP * np.arange(4, dtype=np.int64)
    for j in range(5):
        if j == FAILED:
            continue
        _, states = ev.trajectory(res._traj_rows[res.runs[j].index])
        for s, st in enumerate((near, far)):
            for p, param in enumerate(ALL):
                np.testing.assert_array_equal(views.values[s, p, :, j], stn.aer_value(param, states, q, st))
    np.testing.assert_array_equal(views.of(far, A.Range), views.values[1, 2])
    np.testing.assert_array_equal(views.of(0, A.Visible), views.values[0, 5])
    # the share of the runs holding a sample that see it: formed on the host, over the four good runs
    for s, st in enumerate((near, far)):
        frac = views.visible_fraction(st)
        assert frac.shape == (4,) and ((frac >= 0.0) & (frac <= 1.0)).all()
        np.testing.assert_array_equal(frac, views.values[s, 5][:, [0, 1, 2, 4]].sum(axis=1) / 4.0)
        np.testing.assert_array_equal(views.visible_fraction(s), frac)
    assert views.visible_fraction(near)[0] == 1.0 and (views.visible_fraction(far) == 0.0).all()
    # the same from the elevation alone; the default set is what a one-way measurement reads
    four = res.station_views([near, far], STEP)
    assert four.params == [A.Azimuth, A.Elevation, A.Range, A.RangeRate]
    np.testing.assert_array_equal(four.values, views.values[:, :4])
    np.testing.assert_array_equal(four.visible_fraction(near), views.visible_fraction(near))
    with pytest.raises(ValueError, match="Visible"):
        res.station_views([near], STEP, [A.Range]).visible_fraction(0)
    # a window: two samples, half a step off the grid
    w = res.station_views([far, near], STEP, [A.Range], EPOCH0_NS + STEP // 2, EPOCH0_NS + 2 * STEP)
    assert w.values.shape == (2, 1, 2, 5) and list(w.len) == [0 if j == FAILED else 2 for j in range(5)]
    assert w.epoch0_ns[0] == EPOCH0_NS + STEP // 2
    # bad requests
    with pytest.raises(ValueError, match="window"):
        res.station_views([near], STEP, start_ns=EPOCH0_NS)
    with pytest.raises(ValueError, match="positive step"):
        res.station_views([near], 0)
    with pytest.raises(TypeError):
        res.station_views([near], STEP, [G.Latitude])
    with pytest.raises(ValueError, match="at least one station"):
        res.station_views([], STEP)
    with pytest.raises(ValueError, match="at least one parameter"):
        res.station_views([near], STEP, [])
    with pytest.raises(NotImplementedError):
        res.station_views([nx.GroundStation("moon", 0.0, 0.0, 0.0, nx.Frame(nx.EARTH, ephem.MU_EARTH, A_KM, nx.Rotation(euler=object()), F))], STEP)


def test_traj_aer_splits_parameters_by_eight_and_stations_by_sixteen():
    """GpuContext.traj_aer with a recording stand-in for the library: nine parameters x seventeen stations take four launches, every
    query carries the frame as an event carries it, and the pieces land where the layout says."""
    calls = []

    def fake(handle, traj, n, q, cap, values, length):
        q = q._obj
        calls.append((q.n_stations, q.n_params, list(q.param[:q.n_params]), [q.stations[k].latitude_deg for k in range(q.n_stations)],
                      q.has_frame, q.frame.kind, q.frame_eq_radius_km, q.frame_flattening, q.step_ns, q.has_window, q.start_ns, q.end_ns, cap))
        out = np.ctypeslib.as_array(values, shape=(q.n_stations, q.n_params, cap, n))
        for s in range(q.n_stations):
            for p in range(q.n_params):
                out[s, p] = 1000.0 * q.stations[s].latitude_deg + q.param[p]
        np.ctypeslib.as_array(length, shape=(n,))[:] = cap
        return 0

    import types
    stub = types.SimpleNamespace(_lib=types.SimpleNamespace(nyx_hip_traj_aer=fake), _h=None,
                                 compiled=types.SimpleNamespace(central=types.SimpleNamespace(naif_id=nx.EARTH)))
    t = _abi.TrajBatch(3, 4)
    t.len[:] = 4
    t.epoch_ns[:] = (EPOCH0_NS + STEP * np.arange(4, dtype=np.int64))[:, None]
    sts = [nx.GroundStation(f"s{k}", float(k), 10.0 * k, 0.0, IAU_EARTH, 1.0) for k in range(17)]
    values, length = nx.GpuContext.traj_aer(stub, t, sts, ALL, STEP)
    assert values.shape == (17, 9, 4, 3) and (length == 4).all()
    assert [(c[0], c[1]) for c in calls] == [(16, 8), (16, 1), (1, 8), (1, 1)]
    assert calls[0][2] == list(range(8)) and calls[1][2] == [8] and calls[2][3] == [16.0]
    assert all(c[4:9] == (1, _abi.ROT_IAU, A_KM, F, STEP) and c[9] == 0 and c[12] == 4 for c in calls)
    for s in range(17):
        for p in range(9):
            assert (values[s, p] == 1000.0 * s + p).all()
    calls.clear()
    nx.GpuContext.traj_aer(stub, t, sts[:2], [A.Range], STEP, EPOCH0_NS, EPOCH0_NS + STEP, capacity=7)
    assert len(calls) == 1 and calls[0][9:] == (1, EPOCH0_NS, EPOCH0_NS + STEP, 7)
    with pytest.raises(ValueError, match="window"):
        nx.GpuContext.traj_aer(stub, t, sts[:2], [A.Range], STEP, start_ns=EPOCH0_NS)
    with pytest.raises(NotImplementedError, match="same centre"):
        stub.compiled.central.naif_id = nx.MOON
        nx.GpuContext.traj_aer(stub, t, sts[:2], [A.Range], STEP)
