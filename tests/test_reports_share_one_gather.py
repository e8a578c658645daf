"""CPU: `Results.values_of`, `Results.ric_dispersions`, `Results.ground_tracks`, `Results.station_views` and `Results.eclipses` end in
one gather (`Results._gather_series`, nyx_amd/mc.py).  The five reports of one small ensemble - five runs, one of them failed, four
samples each - with the injected evaluator of tests/test_ric_host.py / tests/test_groundtrack_host.py (the oracle: no fused entry,
every report by composition; `compiled` for the almanac and the centre the eclipses need) must agree on what the gather makes:
`len`, `epoch0_ns` and `ok`; the failed run's column is each report's fill value."""
import numpy as np

import nyx_amd as nx
import oracle_lib
from nyx_amd import ephem
from nyx_amd.eclipse import EclipseParameter as E
from nyx_amd.groundtrack import GroundTrackParameter as G
from nyx_amd.stations import AerParameter as A
from scenarios import EPOCH0_NS, leo_full_setup, leo_nominal

S = nx.NS_PER_S
STEP = 60 * S
IAU_EARTH = nx.Frame(nx.EARTH, ephem.MU_EARTH, 6378.1363, nx.IAU_EARTH_ROTATION, 1.0 / 298.257)
STATIONS = [nx.GroundStation("Madrid", 40.427222, 4.250556, 0.834939, IAU_EARTH, 5.0),
            nx.GroundStation("Canberra", -35.398333, 148.981944, 0.691750, IAU_EARTH, 5.0)]
FAILED = 3


class OracleTraj:
    traj_at = staticmethod(oracle_lib.traj_at)
    traj_every = staticmethod(oracle_lib.traj_every)

    def __init__(self, compiled):
        self.compiled = compiled


def test_the_five_reports_agree_on_len_epoch0_and_ok():
    prop, almanac, central = leo_full_setup(degree=4)
    compiled = prop.compile(almanac, central)
    template = nx.Spacecraft(EPOCH0_NS, leo_nominal(), central, dry_mass_kg=100.0, prop_mass_kg=10.0, srp_area_m2=1.0, cr=1.8)
    mvn = nx.MvnSpacecraft.from_sigmas(template, [1.0, 1.0, 1.0, 1e-3, 1e-3, 1e-3])

    def fn(batch, end_epoch_ns):
        out, st, traj = oracle_lib.propagate_with_traj(compiled, batch, end_epoch_ns - int(batch.epoch_ns[0]), 256)
        st.status[FAILED] = nx._abi.ERR_NAN
        return out, st, traj, OracleTraj(compiled)

    duration = 3 * STEP                                                        # samples at 0, 60, 120 and 180 s: four
    res = nx.MonteCarlo(mvn, seed=3, propagate_fn=fn).run_until_epoch(prop, almanac, EPOCH0_NS + duration, 5)
    nominal = oracle_lib.propagate_with_traj(compiled, nx.pack_spacecraft([template], False), duration, 256)[2]
    assert isinstance(res.runs[FAILED].result, nx.PropagationError)

    vs = res.values_of([nx.StateParameter.X, nx.StateParameter.Rmag, nx.StateParameter.Cr], STEP, value_if_run_failed=-7.0)
    rs = res.ric_dispersions(nominal, STEP)
    gs = res.ground_tracks(IAU_EARTH, STEP, [G.Latitude, G.Longitude])
    av = res.station_views(STATIONS, STEP, [A.Azimuth, A.Elevation, A.Range])
    assert av.values.shape == (2, 3, 4, 5)
    av.values = av.values.reshape(6, 4, 5)                                     # (S * P rows, as the gather saw them)
    es = res.eclipses(nx.ShadowModel.cislunar(almanac), STEP, [E.Occultation, E.State])
    good = [j for j in range(5) if j != FAILED]
    want_len = [0 if j == FAILED else 4 for j in range(5)]
    for series, rows in ((vs, 3), (rs, 6), (gs, 2), (av, 6), (es, 2)):
        assert series.values.shape == (rows, 4, 5)
        assert series.len.dtype == np.int32 and list(series.len) == want_len
        assert series.epoch0_ns.dtype == np.int64 and list(series.epoch0_ns) == [0 if j == FAILED else EPOCH0_NS for j in range(5)]
        assert series.ok.dtype == bool and list(series.ok) == [j != FAILED for j in range(5)]
        assert np.isfinite(series.values[:, :, good]).all()
    for other in (rs, gs, av, es):
        np.testing.assert_array_equal(other.len, vs.len)
        np.testing.assert_array_equal(other.epoch0_ns, vs.epoch0_ns)
        np.testing.assert_array_equal(other.ok, vs.ok)
    # the failed run: the caller's substitute in the list-shaped report, NaN in the other four (and NaN there when none is given)
    assert (vs.values[:, :, FAILED] == -7.0).all()
    assert all(np.isnan(other.values[:, :, FAILED]).all() for other in (rs, gs, av, es))
    assert np.isnan(res.values_of([nx.StateParameter.X], STEP).values[:, :, FAILED]).all()
    assert (rs.count == 4).all()
