"""GPU: the ensemble statistics of a report (include/nyx_hip_stats.h, csrc/stats_kernel.hip) against their definition
(nyx_amd/stats.py).

TOLERANCES.  Bit for bit: HELD, COUNT, MIN, MAX, ARGMIN, ARGMAX, FINITE, SHIFT and every quantile - the selection is exact and
the quantile formula one sequence of rounded operations on both sides (every NaN the library writes is 0x7FF8000000000000, the
NaN of numpy).  SUM within FINITE * 2^-53 * sum |d| and SUMSQ within FINITE * 2^-53 * sum d^2 of the `math.fsum` value: the
classical bound of any summation order (tests/stats_cases.py `compare`).

SYNTHETIC BLOCKS through nyx_hip_series_stats: 3 x 5 at n in {1, 2, 63, 64, 65, 255, 256, 257, 1000} with the adversarial
patterns of tests/test_stats_host.py (NaN sprinkled, a row of NaN, +-inf, -0.0 against +0.0, all values equal, heavy ties,
len 0 and above the capacity, status removing the first run), and one 1 x 2 block each at STAT_LDS_KEYS - 1, STAT_LDS_KEYS and
STAT_LDS_KEYS + 1 runs: the only sizes at which the second key source (the row in global memory) can go wrong.

THE SEVEN KINDS on the family's 70-run, 91-sample LEO ensemble (`leo_full_setup(degree=8)`, `dispersed_leo_batch(70, seed=11)`):
the fused entry equals the definition applied to that report's own host-flavour values, one run failed through `status`."""
import ctypes as C
import dataclasses
import os
import re

import numpy as np
import pytest

import nyx_amd as nx
from nyx_amd import _abi, ephem
from nyx_amd import stats as st
from nyx_amd.eclipse import EclipseParameter as E
from nyx_amd.frames import FrameParameter as F
from nyx_amd.groundtrack import GroundTrackParameter as G
from nyx_amd.links import LinkParameter as L
from nyx_amd.mc import SERIES_REPORTS
from nyx_amd.propagator import report_param_code
from nyx_amd.stations import AerParameter as A
from nyx_amd.stats import Stat
from scenarios import EPOCH0_NS, dispersed_leo_batch, leo_full_setup, leo_nominal
from stats_cases import adversarial_block, big_block, block_probs, canonical_bits, compare

pytestmark = pytest.mark.gpu

S = nx.NS_PER_S
STEP = 60 * S
DUR = 5400 * S
COUNT = 91
STAT_LDS_KEYS = int(re.search(r"#define STAT_LDS_KEYS (\d+)", open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nyx_amd", "csrc",
                                                                                   "stats_args.h")).read()).group(1))
BAND = (0.01, 0.5, 0.99)
IAU_EARTH = nx.Frame(nx.EARTH, ephem.MU_EARTH, 6378.1363, nx.IAU_EARTH_ROTATION, 1.0 / 298.257)
FAILED = 7                # the run every fused test fails through `status`


@pytest.fixture(scope="module")
def world():
    prop, almanac, central = leo_full_setup(degree=8)
    compiled = prop.compile(almanac, central)
    ctx = nx.GpuContext(compiled)
    yield dict(prop=prop, almanac=almanac, central=central, compiled=compiled, ctx=ctx, moon=almanac.frame_info(nx.MOON))
    ctx.close()


@pytest.fixture(scope="module")
def leo70(world):
    """One orbit of 70 dispersed runs, the nominal and the retrograde nominal with dense output: computed once, shared, never written to."""
    ctx = world["ctx"]
    _, stt, traj = ctx.propagate_with_traj(dispersed_leo_batch(70, seed=11), DUR, capacity=256)
    assert (stt.status == 0).all()
    nominal = dispersed_leo_batch(1, seed=0)
    nominal.set_rv(leo_nominal()[None, :])
    _, stt, ref = ctx.propagate_with_traj(nominal, DUR, capacity=256)
    back = nominal.copy()
    back.set_rv(nominal.rv() * np.array([1.0, 1.0, 1.0, -1.0, -1.0, -1.0])[None, :])
    _, stb, tx = ctx.propagate_with_traj(back, DUR, capacity=256)
    assert (stt.status == 0).all() and (stb.status == 0).all()
    status = np.zeros(70, dtype=np.int32)
    status[FAILED] = 3
    for a in (traj.state, traj.epoch_ns, traj.len, status):
        a.setflags(write=False)
    return dict(traj=traj, ref=ref, tx=tx, status=status)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1000])
def test_1_synthetic_blocks_with_every_adversarial_pattern(world, n):
    v, length, status = adversarial_block(n)
    probs = block_probs(length, 5, 4)                                              # (one of them an integral rank at the tie sample)
    for stt in (None, status):
        got = world["ctx"].series_stats(v, length, probs, status=stt)
        compare(got, st.series_stats(v, length, probs, status=stt), v, length, stt, f"n = {n}")
    again = world["ctx"].series_stats(v, length, probs, status=status)
    assert (canonical_bits(again) == canonical_bits(got)).all()                      # the same call twice: the same bits in every column


@pytest.mark.parametrize("n", [STAT_LDS_KEYS - 1, STAT_LDS_KEYS, STAT_LDS_KEYS + 1])
def test_2_both_key_sources_at_the_lds_limit(world, n):
    v, length, status = big_block(n)
    probs = block_probs(length, 2, 1, status)
    got = world["ctx"].series_stats(v, length, probs, status=status)
    compare(got, st.series_stats(v, length, probs, status=status), v, length, status, f"n = {n}")
    assert (canonical_bits(world["ctx"].series_stats(v, length, probs, status=status)) == canonical_bits(got)).all()


def test_3_no_run_no_probability_and_guard_words(world):
    lib, ctx = _abi.load_library(), world["ctx"]
    # n = 0: the empty pattern in a buffer the caller never cleared, nothing behind it touched
    rows, cap, guard = 2, 3, 64
    q = _abi.stats_query((0.5, 1.0))
    out = np.full(rows * cap * 12 + guard, 12345.0)
    assert lib.nyx_hip_series_stats(ctx._h, None, None, None, rows, cap, 0, C.byref(q), out.ctypes.data_as(_abi.c_double_p)) == 0, _abi.last_error()
    got = out[:rows * cap * 12].reshape(rows, cap, 12)
    assert (got[:, :, [0, 1, 6, 7, 8, 9]] == 0).all() and (got[:, :, [4, 5]] == -1).all() and np.isnan(got[:, :, [2, 3, 10, 11]]).all()
    assert (out[rows * cap * 12:] == 12345.0).all()
    # no probability: ten columns; guard words behind them
    v, length, status = adversarial_block(65)
    q0 = _abi.stats_query(())
    out = np.full(3 * 5 * 10 + guard, 12345.0)
    assert lib.nyx_hip_series_stats(ctx._h, v.ctypes.data_as(_abi.c_double_p), length.ctypes.data_as(_abi.c_int32_p), status.ctypes.data_as(_abi.c_int32_p),
                                    3, 5, 65, C.byref(q0), out.ctypes.data_as(_abi.c_double_p)) == 0, _abi.last_error()
    compare(out[:150].reshape(3, 5, 10), st.series_stats(v, length, (), status=status), v, length, status, "no probability")
    assert (out[150:] == 12345.0).all()
    # and with eight of them
    q8 = _abi.stats_query(block_probs(length, 5, 4))
    out = np.full(3 * 5 * 18 + guard, 12345.0)
    assert lib.nyx_hip_series_stats(ctx._h, v.ctypes.data_as(_abi.c_double_p), length.ctypes.data_as(_abi.c_int32_p), None,
                                    3, 5, 65, C.byref(q8), out.ctypes.data_as(_abi.c_double_p)) == 0, _abi.last_error()
    compare(out[:270].reshape(3, 5, 18), st.series_stats(v, length, block_probs(length, 5, 4)), v, length, None, "eight probabilities")
    assert (out[270:] == 12345.0).all()


def test_4_device_pointers_on_a_stream_behind_traj_values(world, leo70):
    """nyx_hip_traj_values_device -> nyx_hip_series_stats_device on one HIP stream, every buffer a device tensor: the same bits as the
    host flavour on the host flavour's values, nothing written beyond rows * capacity * (10 + n_probs) doubles."""
    import torch
    ctx, lib, traj = world["ctx"], _abi.load_library(), leo70["traj"]
    dev = torch.device("cuda", 0)
    n, cap, guard = 70, COUNT, 256
    params = [nx.StateParameter.X, nx.StateParameter.SemiMajorAxis, nx.StateParameter.Inclination]
    values, length = ctx.traj_values(traj, params, STEP, capacity=cap)
    host = ctx.series_stats(values, length, BAND, status=leo70["status"])
    t = {"epoch": torch.tensor(traj.epoch_ns, device=dev), "state": torch.tensor(traj.state, device=dev), "len": torch.tensor(traj.len, device=dev)}
    s = _abi.Traj()
    s.capacity = traj.capacity
    s.epoch_ns = C.cast(t["epoch"].data_ptr(), _abi.c_int64_p)
    for k, f in enumerate(["x_km", "y_km", "z_km", "vx_km_s", "vy_km_s", "vz_km_s"]):
        setattr(s, f, C.cast(t["state"][k].data_ptr(), _abi.c_double_p))
    s.len = C.cast(t["len"].data_ptr(), _abi.c_int32_p)
    q = _abi.ValuesQuery()
    q.n_params, q.step_ns = 3, STEP
    q.param[:3] = [report_param_code(p) for p in params]
    sq = _abi.stats_query(BAND)
    size = 3 * cap * 13
    d_values = torch.zeros(3 * cap * n, dtype=torch.float64, device=dev)
    d_len = torch.zeros(n, dtype=torch.int32, device=dev)
    d_status = torch.tensor(leo70["status"], device=dev)
    d_stats = torch.full((size + guard,), 12345.0, dtype=torch.float64, device=dev)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        h = C.c_void_p(stream.cuda_stream)
        assert lib.nyx_hip_traj_values_device(ctx._h, C.byref(s), n, C.byref(q), cap, C.c_void_p(d_values.data_ptr()), C.c_void_p(d_len.data_ptr()), h) == 0
        rc = lib.nyx_hip_series_stats_device(ctx._h, C.c_void_p(d_values.data_ptr()), C.c_void_p(d_len.data_ptr()), C.c_void_p(d_status.data_ptr()),
                                             3, cap, n, C.byref(sq), C.c_void_p(d_stats.data_ptr()), h)
    assert rc == 0, _abi.last_error()
    stream.synchronize()
    got = d_stats.cpu().numpy()
    assert (canonical_bits(got[:size].reshape(3, cap, 13)) == canonical_bits(host)).all()
    assert (got[size:] == 12345.0).all() and (host[:, :, Stat.HELD] == 69).all() and ctx.last_kernel_ms() > 0.0


def kinds(world, leo70):
    """name -> (the host flavour's (values, len), the same call with stats=)."""
    ctx, traj = world["ctx"], leo70["traj"]
    stations = [nx.GroundStation("A", 10.0, 20.0, 0.5, IAU_EARTH, 5.0), nx.GroundStation("B", -30.0, 100.0, 0.1, IAU_EARTH, 5.0)]
    model = nx.ShadowModel.cislunar(world["almanac"])
    sp = nx.StateParameter
    return {
        "values": lambda **kw: ctx.traj_values(traj, [sp.X, sp.Y, sp.Z, sp.VX, sp.SemiMajorAxis, sp.Eccentricity, sp.Inclination, sp.Rmag, sp.Vmag], STEP, capacity=COUNT, **kw),
        "ground_track": lambda **kw: ctx.traj_ground_track(traj, IAU_EARTH, [G.Latitude, G.Longitude, G.Height], STEP, capacity=COUNT, **kw),
        "aer": lambda **kw: ctx.traj_aer(traj, stations, [A.Azimuth, A.Elevation, A.Range], STEP, capacity=COUNT, **kw),
        "eclipse": lambda **kw: ctx.traj_eclipse(traj, model, [E.Occultation, E.State, E.SunRange], STEP, capacity=COUNT, **kw),
        "frame_values": lambda **kw: ctx.traj_frame_values(traj, world["moon"], [F.Rmag, F.Vmag, F.C3], STEP, capacity=COUNT, **kw),
        "link": lambda **kw: ctx.traj_link(traj, leo70["tx"], [L.Range, L.RangeRate, L.Visible, L.Clearance], STEP, capacity=COUNT, **kw),
        "ric_diff": lambda **kw: ctx.traj_ric_diff(traj, leo70["ref"], STEP, capacity=COUNT, **kw),
    }


@pytest.mark.parametrize("kind", ["values", "ground_track", "aer", "eclipse", "frame_values", "link", "ric_diff"])
def test_5_the_fused_entry_of_every_kind(world, leo70, kind):
    call = kinds(world, leo70)[kind]
    plain = call()
    values, length = plain[0], plain[1]
    fused = call(stats=st.Request(BAND, leo70["status"]))
    assert len(fused) == (3 if kind in ("link", "ric_diff") else 2)
    np.testing.assert_array_equal(fused[1], length)
    if len(fused) == 3:
        np.testing.assert_array_equal(fused[2], plain[2])
    flat = values.reshape(-1, COUNT, 70)
    assert fused[0].shape == values.shape[:-1] + (13,) and (length == COUNT).all()
    want = st.series_stats(flat, length, BAND, status=leo70["status"])
    compare(fused[0].reshape(-1, COUNT, 13), want, flat, length, leo70["status"], kind)
    assert (want[:, :, Stat.HELD] == 69).all() and not (want[:, :, [Stat.ARGMIN, Stat.ARGMAX]] == FAILED).any()
    np.testing.assert_array_equal(call()[0], values)                                # without the keyword: as before


def test_6_the_fused_entry_refuses_through_the_library(world, leo70):
    lib, ctx, traj = _abi.load_library(), world["ctx"], leo70["traj"]
    cin, cref = traj.as_c(), leo70["ref"].as_c()
    q = _abi.ValuesQuery()
    q.n_params, q.step_ns = 1, STEP
    sq = _abi.stats_query(BAND)
    out, length = np.full(COUNT * 13, 12345.0), np.full(70, -7, dtype=np.int32)
    tail = (COUNT, None, C.byref(sq), out.ctypes.data_as(_abi.c_double_p), length.ctypes.data_as(_abi.c_int32_p), None)
    fn = lib.nyx_hip_traj_series_stats
    assert fn(ctx._h, 9, C.byref(cin), 70, None, 0, C.byref(q), C.sizeof(q), *tail) == 1 and "kind = 9" in _abi.last_error()
    assert fn(ctx._h, _abi.SERIES_VALUES, C.byref(cin), 70, None, 0, C.byref(q), C.sizeof(q) + 8, *tail) == 1 and "query_size" in _abi.last_error()
    assert fn(ctx._h, _abi.SERIES_VALUES, C.byref(cin), 70, C.byref(cref), 1, C.byref(q), C.sizeof(q), *tail) == 1 and "takes no second batch" in _abi.last_error()
    rq = _abi.RicQuery()
    rq.step_ns = STEP
    assert fn(ctx._h, _abi.SERIES_RIC, C.byref(cin), 70, None, 0, C.byref(rq), C.sizeof(rq), *tail) == 1 and "needs a second batch" in _abi.last_error()
    q.param[0] = 999                                                               # the report's own refusal, in its own words
    assert fn(ctx._h, _abi.SERIES_VALUES, C.byref(cin), 70, None, 0, C.byref(q), C.sizeof(q), *tail) == 1
    assert _abi.last_error() == "traj_values: param[0] = 999 is not a nyx_hip_state_param"
    assert (out == 12345.0).all() and (length == -7).all()                          # nothing was launched


def test_7_results_series_stats_fused_against_composed(world, leo70):
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
    assert isinstance(res.runs[fail].result, nx.PropagationError)
    ctx = res._traj_ctx

    class Compose:   # the evaluator of the definition: traj_every / traj_at only, and what the runs were compiled from
        traj_at = staticmethod(ctx.traj_at)
        traj_every = staticmethod(ctx.traj_every)
        compiled = ctx.compiled

    composed = dataclasses.replace(res, _traj_ctx=Compose)
    sp = nx.StateParameter
    for report, args in (("values_of", ([sp.X, sp.SemiMajorAxis, sp.Inclination], STEP)), ("link_views", (leo70["tx"], STEP, [L.Range, L.Visible])),
                         ("ric_dispersions", (leo70["ref"], STEP)), ("station_views", ([nx.GroundStation("A", 10.0, 20.0, 0.5, IAU_EARTH, 5.0)], STEP, [A.Elevation]))):
        calls = []
        entry = SERIES_REPORTS[report]
        real = getattr(ctx, entry)
        ctx.__dict__[entry] = lambda *a, _real=real, **kw: (calls.append(kw.get("stats")), _real(*a, **kw))[1]
        try:
            got = res.series_stats(report, *args, probs=BAND)
        finally:
            del ctx.__dict__[entry]
        assert len(calls) == 1 and calls[0] is not None, report                     # the fused path was taken, once
        # the definition applied to that report's own values (the composition `series_stats` falls back to), by the tolerances above
        series = getattr(res, report)(*args)
        flat = series.values.reshape(len(got.rows), COUNT, runs)
        failed = (~series.ok).astype(np.int32)
        assert isinstance(got, nx.SeriesStats) and got.probs == BAND and got.stats.shape == (len(got.rows), COUNT, 13), report
        compare(got.stats, st.series_stats(flat, series.len, BAND, status=failed), flat, series.len, failed, report)
        assert (got.of(Stat.HELD) == runs - 1).all() and got.epochs()[0] == EPOCH0_NS and got.epochs()[1] == EPOCH0_NS + STEP
        want = composed.series_stats(report, *args, probs=BAND)                     # an evaluator without the fused entries: composed
        assert got.rows == want.rows and want.stats.shape == got.stats.shape and (want.epochs() == got.epochs()).all()
        for c in (Stat.HELD, Stat.COUNT, Stat.FINITE):
            np.testing.assert_array_equal(got.of(c), want.of(c))
        if report == "link_views":                                                  # (the report whose device values equal the composition bit for bit)
            compare(got.stats, want.stats, flat, series.len, failed, "link_views, composed evaluator")
    # a dispersed constant of the run does not come from the device: composed, on a device evaluator too
    mixed = res.series_stats("values_of", [sp.X, sp.Cr], STEP, probs=BAND)
    assert mixed.stats.shape == (2, COUNT, 13) and (mixed.of(Stat.MIN)[1] == mixed.of(Stat.MAX)[1]).all()
