"""CPU: `Results.series_stats` by composition - the injected CPU evaluators of tests/test_mc_results.py have no fused entry, so the
named report runs as it always did and nyx_amd/stats.py reduces its values: a failed run is left out, the rows and epochs are the
report's, a sharded pair of ranks on gloo gives the same SeriesStats on both ranks as one process, and without the `stats=` keyword
the seven `GpuContext.traj_*` methods and `_param_series` return what they returned before."""
import ctypes as C
import inspect
import os
import sys

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

import nyx_amd as nx
from nyx_amd import _abi
from nyx_amd import stats as st
from nyx_amd.params import StateParameter as P
from nyx_amd.propagator import _param_series
from nyx_amd.stats import Stat
from scenarios import EPOCH0_NS

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from stats_cases import canonical_bits  # noqa: E402
from test_distributed_cpu import _build_with_traj, _free_port  # noqa: E402
from test_mc_results import _mc  # noqa: E402

STEP = 300 * nx.NS_PER_S
BAND = (0.01, 0.5, 0.99)


def test_series_stats_is_the_report_then_the_definition_and_leaves_a_failed_run_out():
    prop, almanac, compiled, mc = _mc(fail_index=2)
    res = mc.run_until_epoch(prop, almanac, EPOCH0_NS + 1800 * nx.NS_PER_S, 6)
    assert isinstance(res.runs[2].result, nx.PropagationError) and not hasattr(res._traj_ctx, "traj_values")
    params = [P.X, P.Rmag, P.Cr]
    got = res.series_stats("values_of", params, STEP, probs=BAND)
    series = res.values_of(params, STEP)
    want = st.series_stats(series.values, series.len, BAND, status=(~series.ok).astype(np.int32))
    assert isinstance(got, nx.SeriesStats) and got.rows == params and got.probs == BAND and got.stats.shape == (3, 7, 13)
    assert (canonical_bits(got.stats) == canonical_bits(want)).all()
    assert (got.of(Stat.HELD) == 5).all() and (got.of(Stat.COUNT) == 5).all() and not (got.stats[:, :, [Stat.ARGMIN, Stat.ARGMAX]] == 2).any()
    assert got.epochs().tolist() == [EPOCH0_NS + k * STEP for k in range(7)] and got.step_ns == STEP
    ok = np.nonzero(series.ok)[0]
    x = series.values[:, :, ok]
    np.testing.assert_array_equal(got.of(Stat.MIN), x.min(axis=2))
    np.testing.assert_array_equal(got.of(Stat.MAX), x.max(axis=2))
    np.testing.assert_array_equal(got.of(Stat.ARGMIN), ok[x.argmin(axis=2)])
    np.testing.assert_array_equal(got.quantile(1), np.quantile(x, 0.5, axis=2))                  # (m = 5: the middle one, an order statistic)
    # (mean and sigma of five values near 7000 km / 1 km: a few ulp of 7000 either way)
    np.testing.assert_allclose(got.mean(), x.mean(axis=2), rtol=0, atol=8 * np.spacing(7000.0))
    # (sigma ~ 1 km from SUMSQ - SUM^2 / n with |d| ~ 1: no cancellation to speak of, 1e-9 is six digits above either side's rounding)
    np.testing.assert_allclose(got.std()[:2], x.std(axis=2, ddof=1)[:2], rtol=1e-9)
    assert (got.of(Stat.MIN)[2] == 1.8).all() and (got.std()[2] == 0).all()                      # Cr: a constant of the runs
    # a value for the failed run does not enter either: its len is 0
    filled = res.series_stats("values_of", params, STEP, probs=BAND, value_if_run_failed=-1.0)
    assert (canonical_bits(filled.stats) == canonical_bits(got.stats)).all()
    # windowed, and another report through the same door: the RIC dispersions about run 0
    win = res.series_stats("values_of", [P.X], STEP, EPOCH0_NS + STEP, EPOCH0_NS + 3 * STEP, probs=())
    assert win.stats.shape == (1, 3, 10) and win.epochs()[0] == EPOCH0_NS + STEP
    ric = res.series_stats("ric_dispersions", res.runs[0].result.traj, STEP, probs=BAND)
    rs = res.ric_dispersions(res.runs[0].result.traj, STEP)
    assert ric.rows == ["dR", "dI", "dC", "dvR", "dvI", "dvC"] and ric.stats.shape == (6, 7, 13)
    assert (canonical_bits(ric.stats) == canonical_bits(st.series_stats(rs.values, rs.len, BAND, status=(~rs.ok).astype(np.int32)))).all()
    np.testing.assert_array_equal(ric.of(Stat.HELD)[0], rs.count)
    with pytest.raises(ValueError, match="report must be one of"):
        res.series_stats("every_value_of", P.X, STEP)
    with pytest.raises(nx.StateError):
        res.series_stats("values_of", [P.Isp], STEP)


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    prop, almanac, mc = _build_with_traj(11)
    res = mc.resume_run_until_epoch(prop, almanac, 0, EPOCH0_NS + 900 * nx.NS_PER_S, 7, dist=dist)
    got = res.series_stats("values_of", [P.X, P.Rmag], STEP, probs=BAND)
    np.savez(os.path.join(out_dir, f"s{rank}.npz"), stats=got.stats, epochs=got.epochs(), n_local=len(res._local_runs()))
    dist.destroy_process_group()


def test_a_sharded_pair_of_ranks_gives_the_same_statistics_on_both(tmp_path):
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    a, b = np.load(tmp_path / "s0.npz"), np.load(tmp_path / "s1.npz")
    assert int(a["n_local"]) + int(b["n_local"]) == 7 and int(a["n_local"]) < 7
    assert (canonical_bits(a["stats"]) == canonical_bits(b["stats"])).all() and (a["epochs"] == b["epochs"]).all()
    prop, almanac, mc = _build_with_traj(11)
    single = mc.run_until_epoch(prop, almanac, EPOCH0_NS + 900 * nx.NS_PER_S, 7).series_stats("values_of", [P.X, P.Rmag], STEP, probs=BAND)
    assert (canonical_bits(a["stats"]) == canonical_bits(single.stats)).all() and a["stats"].shape == (2, 4, 13)
    assert (single.of(Stat.HELD) == 7).all()


def test_without_the_keyword_every_method_returns_what_it_returned():
    for name in _abi.SERIES_KINDS:
        assert inspect.signature(getattr(nx.GpuContext, name)).parameters["stats"].default is None, name
    assert inspect.signature(_param_series).parameters["stats"].default is None
    traj = _abi.TrajBatch(3, 4)
    seen = []

    def fake(handle, cin, n, q, cap, values, length):   # a host flavour: writes its parameter codes
        seen.append((n, q._obj.n_params, cap))
        out = np.ctypeslib.as_array(values, shape=(q._obj.n_params * cap * n,)).reshape(q._obj.n_params, cap, n)
        for k in range(q._obj.n_params):
            out[k] = q._obj.param[k]
        np.ctypeslib.as_array(length, shape=(n,))[:] = cap
        return 0

    values, length = _param_series("traj_values", fake, None, _abi.ValuesQuery, _abi.MAX_REPORT_PARAMS, lambda q: None, traj, list(range(10)), 10**9, None, None, 5)
    assert values.shape == (10, 5, 3) and (length == 5).all() and seen == [(3, 8, 5), (3, 2, 5)]
    assert (values == np.arange(10.0)[:, None, None]).all()
    with pytest.raises(ValueError, match="prob"):
        _param_series("traj_values", fake, None, _abi.ValuesQuery, _abi.MAX_REPORT_PARAMS, lambda q: None, traj, [0], 10**9, None, None, 5, stats=(1.5,))
    with pytest.raises(ValueError, match="status holds 2 entries"):
        _param_series("traj_values", fake, None, _abi.ValuesQuery, _abi.MAX_REPORT_PARAMS, lambda q: None, traj, [0], 10**9, None, None, 5,
                      stats=st.Request((0.5,), [0, 1]))
    assert len(seen) == 2 and C.sizeof(_abi.StatsQuery) == 72
