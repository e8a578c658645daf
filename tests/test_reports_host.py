"""`Results.values_of` (the array form of the list reports) on the host: with an injected evaluator (the oracle, as in
tests/test_mc_results.py) it composes `traj_every` / `traj_at` + `state_value`, and must equal the existing list reports
`every_value_of`, `every_value_of_between`, `first_values_of`, `last_values_of` EXACTLY, column by column - failed runs,
clamped and empty windows, the constants of a run and the unavailable parameters included - and gather the columns of a
sharded ensemble in index order.  No GPU here: that composition is the definition the device path is tested against
(tests/test_gpu_reports.py)."""
import os
import socket
import sys

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

import nyx_amd as nx
import oracle_lib
from nyx_amd.params import StateParameter as P
from scenarios import EPOCH0_NS, leo_full_setup, leo_nominal

S = nx.NS_PER_S
STEP = 300 * S
PARAMS = [P.X, P.VZ, P.Rmag, P.SemiMajorAxis, P.Eccentricity, P.TrueAnomaly, P.Cr, P.TotalMass, P.Inclination, P.Period]


class OracleTraj:
    """What Results needs from a context: traj_at / traj_every (GpuContext's signatures); no traj_values."""

    traj_at = staticmethod(oracle_lib.traj_at)
    traj_every = staticmethod(oracle_lib.traj_every)


def _mc(fail_index=None, seed=3):
    prop, almanac, central = leo_full_setup(degree=4)
    compiled = prop.compile(almanac, central)
    template = nx.Spacecraft(EPOCH0_NS, leo_nominal(), central, dry_mass_kg=100.0, prop_mass_kg=10.0, srp_area_m2=1.0, cr=1.8)
    mvn = nx.MvnSpacecraft.from_sigmas(template, [1.0, 1.0, 1.0, 1e-3, 1e-3, 1e-3])

    def fn(batch, end_epoch_ns):
        out, st, traj = oracle_lib.propagate_with_traj(compiled, batch, end_epoch_ns - int(batch.epoch_ns[0]), 256)
        if fail_index is not None:
            st.status[fail_index] = nx._abi.ERR_NAN
        return out, st, traj, OracleTraj

    return prop, almanac, nx.MonteCarlo(mvn, seed=seed, propagate_fn=fn)


def _columns_equal_list(vs, p, listed):
    """The list report is the columns of the successful runs, run after run, each cut at its len."""
    at = 0
    j_param = vs.params.index(p)
    for j in range(vs.values.shape[2]):
        if not vs.ok[j]:
            continue
        n = int(vs.len[j])
        np.testing.assert_array_equal(vs.values[j_param, :n, j], listed[at:at + n], err_msg=f"{p.name}, run {j}")
        assert np.isnan(vs.values[j_param, n:, j]).all()
        at += n
    assert at == len(listed)


def test_values_of_equals_the_four_list_reports():
    prop, almanac, mc = _mc()
    end = EPOCH0_NS + 1800 * S
    res = mc.run_until_epoch(prop, almanac, end, 5)
    vs = res.values_of(PARAMS, STEP)
    assert isinstance(vs, nx.ValueSeries) and vs.values.shape == (len(PARAMS), 7, 5) and vs.step_ns == STEP
    assert vs.len.dtype == np.int32 and (vs.len == 7).all() and vs.ok.all() and (vs.epoch0_ns == EPOCH0_NS).all()
    assert list(vs.epochs(2)) == [EPOCH0_NS + k * STEP for k in range(7)]
    for p in PARAMS:
        listed = res.every_value_of(p, STEP)
        assert len(listed) == 35
        _columns_equal_list(vs, p, listed)
        assert vs.flat(p) == listed
        # sample 0 of a run = first_values_of; 1800 s = 6 steps, so the last sample is the stored end state = last_values_of
        np.testing.assert_array_equal(vs.values[vs.params.index(p), 0, :], res.first_values_of(p))
        np.testing.assert_array_equal(vs.values[vs.params.index(p), 6, :], res.last_values_of(p))
    # last_values_of whatever the step: the window [end, end]
    tail = res.values_of(PARAMS, 7 * S, end, end)
    assert tail.values.shape == (len(PARAMS), 1, 5) and (tail.len == 1).all() and (tail.epoch0_ns == end).all()
    for j, p in enumerate(PARAMS):
        np.testing.assert_array_equal(tail.values[j, 0, :], res.last_values_of(p))
    assert vs.flat(P.Cr) == [1.8] * 35 and vs.flat(P.TotalMass) == [110.0] * 35


def test_failed_run_with_and_without_a_substitute():
    prop, almanac, mc = _mc(fail_index=2)
    res = mc.run_until_epoch(prop, almanac, EPOCH0_NS + 600 * S, 4)
    assert isinstance(res.runs[2].result, nx.PropagationError)
    for sub in (None, -7.5):
        vs = res.values_of([P.Y, P.SemiMajorAxis, P.Cr], STEP, value_if_run_failed=sub)
        assert vs.values.shape == (3, 3, 4) and list(vs.len) == [3, 3, 0, 3] and list(vs.ok) == [True, True, False, True]
        if sub is None:
            assert np.isnan(vs.values[:, :, 2]).all()
        else:
            assert (vs.values[:, :, 2] == sub).all()
        assert vs.epoch0_ns[2] == 0
        for p in (P.Y, P.SemiMajorAxis, P.Cr):
            listed = res.every_value_of(p, STEP, value_if_run_failed=sub)
            assert len(listed) == (9 if sub is None else 10)
            assert vs.flat(p, value_if_run_failed=sub) == listed
            _columns_equal_list(vs, p, res.every_value_of(p, STEP))


def test_windows_that_cut_some_runs_short_and_windows_outside_every_run():
    prop, almanac, mc = _mc()
    end = EPOCH0_NS + 1800 * S
    res = mc.run_until_epoch(prop, almanac, end, 4)
    # run 1 keeps only the first part of its trajectory: it ends before the window does, the others are cut by the window
    tb = res._traj_batch
    row = res._traj_rows[1]
    keep = int(np.searchsorted(tb.epoch_ns[: tb.len[row], row], EPOCH0_NS + 1000 * S))
    assert 2 < keep < tb.len[row]
    tb.len[row] = keep
    last1 = int(tb.epoch_ns[keep - 1, row])
    start, stop = EPOCH0_NS - 10 * STEP, EPOCH0_NS + 1500 * S          # starts before the runs: clamped to their first epoch
    params = [P.X, P.Rmag, P.AoP, P.PropMass]
    vs = res.values_of(params, STEP, start, stop)
    want1 = (last1 - EPOCH0_NS) // STEP + 1
    assert list(vs.len) == [6, want1, 6, 6] and want1 < 6 and vs.values.shape == (4, 6, 4)
    assert (vs.epoch0_ns == EPOCH0_NS).all()
    for p in params:
        listed = res.every_value_of_between(p, STEP, start, stop)
        assert len(listed) == 18 + want1
        _columns_equal_list(vs, p, listed)
    # a window that starts inside the runs
    inside = res.values_of(params, STEP, EPOCH0_NS + 450 * S, end + STEP)
    assert (inside.epoch0_ns == EPOCH0_NS + 450 * S).all() and inside.len[0] == 5
    for p in params:
        _columns_equal_list(inside, p, res.every_value_of_between(p, STEP, EPOCH0_NS + 450 * S, end + STEP))
    # outside every run: no sample at all
    none = res.values_of(params, STEP, end + STEP, end + 3 * STEP)
    assert none.values.shape == (4, 0, 4) and (none.len == 0).all() and none.ok.all()
    assert none.flat(P.X) == res.every_value_of_between(P.X, STEP, end + STEP, end + 3 * STEP) == []


def test_unavailable_parameters_and_bad_requests_raise():
    prop, almanac, mc = _mc()
    res = mc.run_until_epoch(prop, almanac, EPOCH0_NS + 600 * S, 2)
    for p in (P.Isp, P.Thrust):
        with pytest.raises(nx.StateError):
            res.values_of([P.X, p], STEP)
    with pytest.raises(ValueError):
        res.values_of([P.X], STEP, start_ns=EPOCH0_NS)
    res._traj_batch = None
    with pytest.raises(ValueError, match="carry no trajectories"):
        res.values_of([P.X], STEP)


def test_traj_values_every_needs_an_evaluator_with_the_fused_entry():
    """`Traj.values_every` is the device path by definition: an evaluator without `traj_values` is an error, not a fall-back."""
    prop, almanac, mc = _mc()
    res = mc.run_until_epoch(prop, almanac, EPOCH0_NS + 600 * S, 1)
    with pytest.raises(AttributeError):
        res.runs[0].result.traj.values_every([P.X], STEP)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


GATHER_PARAMS = [P.X, P.SemiMajorAxis, P.Cr]


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    prop, almanac, mc = _mc(fail_index=1)          # position 1 of EVERY shard fails: runs 1 and 5 of 7
    res = mc.resume_run_until_epoch(prop, almanac, 0, EPOCH0_NS + 900 * S, 7, dist=dist)
    vs = res.values_of(GATHER_PARAMS, STEP, value_if_run_failed=-1.0)
    win = res.values_of(GATHER_PARAMS, STEP, EPOCH0_NS + 100 * S, EPOCH0_NS + 700 * S)
    outcome = "no error"
    try:
        res.values_of([P.Isp], STEP)
    except nx.StateError as e:
        outcome = "StateError: " + str(e)
    np.savez(os.path.join(out_dir, f"v{rank}.npz"), values=vs.values, len=vs.len, epoch0=vs.epoch0_ns, ok=vs.ok, wvalues=win.values, wlen=win.len,
             wepoch0=win.epoch0_ns, n_local=len(res._local_runs()), outcome=outcome)
    dist.destroy_process_group()


def test_two_rank_gloo_gather_in_index_order(tmp_path):
    port = _free_port()
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    v = [np.load(tmp_path / f"v{r}.npz") for r in range(2)]
    assert [int(x["n_local"]) for x in v] == [4, 3]
    for k in ("values", "len", "epoch0", "ok", "wvalues", "wlen", "wepoch0"):
        np.testing.assert_array_equal(v[0][k], v[1][k])        # every rank holds the complete series (NaN == NaN here)
    assert all(str(x["outcome"]).startswith("StateError") for x in v)
    # == the single-process series of the same seeded ensemble with the same runs failed
    prop, almanac, mc = _mc()
    res = mc.run_until_epoch(prop, almanac, EPOCH0_NS + 900 * S, 7)
    for idx in (1, 5):
        res.runs[idx].result = nx.PropagationError(nx._abi.ERR_NAN, idx)
    vs = res.values_of(GATHER_PARAMS, STEP, value_if_run_failed=-1.0)
    win = res.values_of(GATHER_PARAMS, STEP, EPOCH0_NS + 100 * S, EPOCH0_NS + 700 * S)
    assert list(vs.len) == [4, 0, 4, 4, 4, 0, 4] and vs.values.shape == (3, 4, 7)
    np.testing.assert_array_equal(v[0]["values"], vs.values)
    np.testing.assert_array_equal(v[0]["len"], vs.len)
    np.testing.assert_array_equal(v[0]["epoch0"], vs.epoch0_ns)
    np.testing.assert_array_equal(v[0]["ok"], vs.ok)
    np.testing.assert_array_equal(v[0]["wvalues"], win.values)
    np.testing.assert_array_equal(v[0]["wlen"], win.len)
    assert list(win.len) == [3, 0, 3, 3, 3, 0, 3] and (win.epoch0_ns[vs.ok] == EPOCH0_NS + 100 * S).all()
    assert (vs.values[:, :, 1] == -1.0).all() and np.isnan(win.values[:, :, 5]).all()
