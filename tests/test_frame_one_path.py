"""CPU: the encounter report through the one Python path of the series reports (`Results._series` in nyx_amd/mc.py, `_param_series` in
nyx_amd/propagator.py), the pattern of tests/test_series_one_path.py and its injected evaluators.

* The FUSED branch of `Results.frame_values`, with an evaluator that offers `traj_frame_values` in the entry's layout - NaN past `len`,
  a capacity larger than the longest series - built by composition from `frames.frame_value`: it equals the report through the
  composing evaluator (no fused entry: the definition) bit for bit, with ONE launch counted.  Five runs, one failed, one with a shorter
  trajectory, both windows; the target is the Moon.
* The target set to the Earth itself: nothing is hyperbolic, the B-plane rows are NaN and `len` is what it is about the Moon.
* A sharded ensemble (two gloo ranks, seven runs) equals the single-process result.
* `FrameSeries.closest_approach` / `hyperbolic_fraction` against numpy on the columns; `Traj.to_frame` against `frames.to_frame`.
* The launcher: more than eight parameters split into launches, the chain and mu filled into every query."""
import ctypes as C
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

import nyx_amd as nx
import oracle_lib
from nyx_amd import _abi, eclipse, frames, propagator
from nyx_amd.frames import FrameParameter as F
from scenarios import EPOCH0_NS
from test_ric_host import _free_port
from test_series_one_path import FAILED, FIELDS, SHORT, SPARE, STEP, WINDOWS, Composing, _mc

S = nx.NS_PER_S
PARAMS = [F.Rmag, F.PeriapsisRadius, F.C3, F.BdotT, F.BdotR]


class Fused(Composing):
    """`traj_frame_values` with GpuContext's signature and layout, composed from `traj_every` / `traj_at` and the host definition.
    `calls` counts the launches: a report that quietly took the composition instead would compare the definition with itself."""

    def traj_frame_values(self, tb, target, params, step_ns, start_ns=None, end_ns=None):
        self.calls += 1
        al, central = self.compiled.almanac, self.compiled.central
        lo, hi = propagator.series_bounds(tb, start_ns, end_ns)
        live = np.nonzero(hi >= lo)[0]
        longest = int(((hi[live] - lo[live]) // step_ns).max()) + 1 if len(live) else 1
        values, length = np.full((len(params), longest + SPARE, tb.n), np.nan), np.zeros(tb.n, dtype=np.int32)
        for i in live:
            q = lo[i] + step_ns * np.arange((hi[i] - lo[i]) // step_ns + 1, dtype=np.int64)
            states, status = oracle_lib.traj_at(nx.Traj(None, tb, i)._single(), q)
            end = np.nonzero(_abi.interp_failed(status[:, 0]))[0]
            rv = states[: (end[0] if len(end) else len(q)), 0]
            moved = frames.to_frame(rv, q[:len(rv)], target, al, central)
            end = np.nonzero(np.isnan(moved).any(axis=1))[0]              # (outside the ephemerides: the series ends; a NaN B-plane value does not end it)
            k = int(end[0]) if len(end) else len(rv)
            length[i] = k
            values[:, :k, i] = np.stack([frames.frame_value(p, rv[:k], q[:k], target, al, central) for p in params]).reshape(len(params), k)
        return values, length


@pytest.fixture(scope="module")
def world():
    """(results through the fused evaluator, the same results through the composing one, the Moon, the Earth)."""
    prop, almanac, compiled, template, carlo = _mc(Fused, FAILED, nx.IntegratorOptions.with_fixed_step(20 * S))   # ten stored states in 180 s
    fused = carlo.run_until_epoch(prop, almanac, EPOCH0_NS + 3 * STEP, 5)
    tb, row = fused._traj_batch, fused._traj_rows[fused.runs[SHORT].index]
    keep = int(np.searchsorted(tb.epoch_ns[: tb.len[row], row], EPOCH0_NS + 2 * STEP + 1))    # run SHORT ends between samples 2 and 3
    assert 2 < keep < tb.len[row]
    tb.len[row] = keep
    return fused, dataclasses.replace(fused, _traj_ctx=Composing(compiled)), almanac.frame_info(nx.MOON), compiled.central, almanac


@pytest.mark.parametrize("window", WINDOWS)
def test_the_fused_branch_equals_the_composition(world, window):
    fused, composed, moon = world[:3]
    fused._traj_ctx.calls = composed._traj_ctx.calls = 0
    a = fused.frame_values(moon, PARAMS, STEP, *window)
    assert fused._traj_ctx.calls == 1 and composed._traj_ctx.calls == 0         # one launch ...
    b = composed.frame_values(moon, PARAMS, STEP, *window)
    assert type(a) is type(b) is nx.FrameSeries and dataclasses.fields(a) == dataclasses.fields(b) and a.step_ns == b.step_ns == STEP
    for f in FIELDS:                                                            # ... and the same series, bit for bit
        assert getattr(a, f).dtype == getattr(b, f).dtype
        np.testing.assert_array_equal(getattr(a, f), getattr(b, f))
    assert a.params == PARAMS and a.target is moon
    assert list(a.len) == ([4, 3, 4, 0, 4] if window[0] is None else [3, 2, 3, 0, 3]) and list(a.ok) == [j != FAILED for j in range(5)]
    assert a.values.shape == (5, a.len.max(), 5) and np.isfinite(a.values[:, :a.len[SHORT], SHORT]).all()
    assert np.isnan(a.values[:, a.len[SHORT]:, SHORT]).all() and np.isnan(a.values[:, :, FAILED]).all()
    # every held sample is on a hyperbola about the Moon, some 4e5 km away
    held = np.arange(a.values.shape[1])[:, None] < a.len[None, :]
    assert ((a.of(F.Rmag)[held] > 3.4e5) & (a.of(F.Rmag)[held] < 4.2e5)).all() and (a.of(F.C3)[held] > 0.0).all() and np.isfinite(a.of(F.BdotT)[held]).all()
    # the helpers against numpy on the columns
    k, rmin = a.closest_approach()
    for j in range(5):
        col = a.of(nx.StateParameter.Rmag)[:a.len[j], j]
        assert (k[j], rmin[j]) == (int(np.argmin(col)), col.min()) if a.len[j] else (k[j] == -1 and np.isnan(rmin[j]))
    frac = a.hyperbolic_fraction()
    assert list(frac[a.ok]) == [1.0] * 4 and np.isnan(frac[FAILED])
    with pytest.raises(ValueError, match="does not hold Rmag"):
        fused.frame_values(moon, [F.C3], STEP, *window).closest_approach()
    with pytest.raises(ValueError, match="holds neither"):
        fused.frame_values(moon, [F.C3], STEP, *window).hyperbolic_fraction()


@pytest.mark.parametrize("window", WINDOWS)
def test_the_centre_itself_nan_and_continue(world, window):
    fused, composed, moon, earth = world[:4]
    fused._traj_ctx.calls = 0
    a = fused.frame_values(earth, PARAMS + [F.Eccentricity], STEP, *window)
    b = composed.frame_values(earth, PARAMS + [F.Eccentricity], STEP, *window)
    assert fused._traj_ctx.calls == 1
    for f in FIELDS:
        np.testing.assert_array_equal(getattr(a, f), getattr(b, f))
    np.testing.assert_array_equal(a.len, fused.frame_values(moon, PARAMS, STEP, *window).len)            # `len` is unchanged ...
    held = np.arange(a.values.shape[1])[:, None] < a.len[None, :]
    assert np.isnan(a.of(F.BdotT)).all() and np.isnan(a.of(F.BdotR)).all()                                # ... the B-plane rows are NaN ...
    assert np.isfinite(a.of(F.Rmag)[held]).all() and (a.of(F.C3)[held] < 0.0).all() and (a.of(F.Eccentricity)[held] < 1.0).all()    # ... the others are not
    assert list(a.hyperbolic_fraction()[a.ok]) == [0.0] * 4
    series = fused.frame_values(earth, [F.Eccentricity], STEP, *window)                                   # the eccentricity alone tells, too
    assert list(series.hyperbolic_fraction()[series.ok]) == [0.0] * 4
    # the identity: the values of `values_of` for the parameters the two reports share
    same = composed.values_of([nx.StateParameter.Rmag, nx.StateParameter.PeriapsisRadius], STEP, *window)
    np.testing.assert_array_equal(a.values[:2], same.values)


def test_traj_to_frame_is_the_host_definition(world):
    fused, _, moon, earth, almanac = world
    traj = fused.runs[0].result.traj
    moved = traj.to_frame(moon)
    assert isinstance(moved, nx.Traj) and moved is not traj and len(moved) == len(traj) > 4
    np.testing.assert_array_equal(moved.epochs_ns, traj.epochs_ns)
    np.testing.assert_array_equal(moved.states, frames.to_frame(traj.states, traj.epochs_ns, moon, almanac, earth))
    assert np.linalg.norm(moved.states[:, :3], axis=1).min() > 3.4e5
    np.testing.assert_array_equal(traj.to_frame(earth).states, traj.states)
    # an epoch outside the ephemerides raises
    end_s = min(float(almanac.segments[s].init_et_s) + float(almanac.segments[s].interval_s) * almanac.segments[s].records.shape[0]
                for s, _ in eclipse.body_chain(nx.MOON, almanac, earth))
    late = nx.Traj.from_arrays(traj._ctx, [EPOCH0_NS, int(end_s + 10) * S], traj.states[:2])
    with pytest.raises(ValueError, match="outside the ephemerides"):
        late.to_frame(moon)
    with pytest.raises(KeyError, match="planetary data"):
        traj.to_frame(nx.Frame(499, 42828.0))
    with pytest.raises(ValueError, match="does not know the almanac"):
        nx.Traj.from_arrays(None, traj.epochs_ns, traj.states).to_frame(moon)


# ---- a sharded ensemble ----------------------------------------------------------------------------------------------
END = EPOCH0_NS + 5 * STEP
SHARD_WINDOWS = [(None, None), (EPOCH0_NS + 100 * S, EPOCH0_NS + 250 * S)]


def _sharded_reports(res, almanac):
    moon = almanac.frame_info(nx.MOON)
    return {k: res.frame_values(moon, PARAMS, STEP, *win) for k, win in enumerate(SHARD_WINDOWS)}


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    prop, almanac, _, _, carlo = _mc(Composing, 1)          # position 1 of EVERY shard fails: runs 1 and 5 of 7
    res = carlo.resume_run_until_epoch(prop, almanac, 0, END, 7, dist=dist)
    got = {f"{k}_{f}": getattr(series, f) for k, series in _sharded_reports(res, almanac).items() for f in FIELDS}
    outcome = "no error"
    try:
        res.frame_values(almanac.frame_info(nx.MOON), PARAMS if rank == 0 else [], STEP)    # one rank refuses: both raise, neither waits in a collective
    except (ValueError, RuntimeError) as e:
        outcome = type(e).__name__
    np.savez(os.path.join(out_dir, f"r{rank}.npz"), n_local=len(res._local_runs()), outcome=outcome, **got)
    dist.destroy_process_group()


def test_two_rank_gloo_equals_the_single_process_result(tmp_path):
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    v = [np.load(tmp_path / f"r{r}.npz") for r in range(2)]
    assert [int(x["n_local"]) for x in v] == [4, 3] and [str(x["outcome"]) for x in v] == ["RuntimeError", "ValueError"]
    prop, almanac, _, _, carlo = _mc(Composing, None)
    res = carlo.run_until_epoch(prop, almanac, END, 7)
    for idx in (1, 5):
        res.runs[idx].result = nx.PropagationError(_abi.ERR_NAN, idx)
    for k, series in _sharded_reports(res, almanac).items():
        assert list(series.len) == [0 if j in (1, 5) else (3 if k else 6) for j in range(7)] and series.values.shape == (5, (3 if k else 6), 7)
        for f in FIELDS:
            for rank in range(2):                                              # every rank holds the complete result (NaN == NaN here)
                got = v[rank][f"{k}_{f}"]
                assert got.dtype == getattr(series, f).dtype
                np.testing.assert_array_equal(got, getattr(series, f), err_msg=f"window {k} {f} on rank {rank}")


# ---- the launcher ----------------------------------------------------------------------------------------------------
def test_more_than_eight_parameters_split_into_launches(world):
    """`GpuContext.traj_frame_values` through `_param_series` with a recording callable in place of the ctypes entry."""
    fused, _, moon, earth, almanac = world
    t = _abi.TrajBatch(3, 4)
    t.len[:] = 4
    t.epoch_ns[:] = (EPOCH0_NS + STEP * np.arange(4, dtype=np.int64))[:, None]
    calls = []

    def fake(handle, ctraj, n, q, capacity, values, length):
        q = q._obj
        calls.append((q.n_params, list(q.param[:q.n_params]), q.has_window, q.step_ns, q.n_chain, list(q.chain_segment[:q.n_chain]), list(q.chain_sign[:q.n_chain]),
                      q.mu_km3_s2))
        out = np.ctypeslib.as_array(values, shape=(q.n_params, capacity, n))
        for c in range(q.n_params):
            out[c] = float(q.param[c])
        np.ctypeslib.as_array(length, shape=(n,))[:] = capacity
        return 0

    class Lib:
        nyx_hip_traj_frame_values = staticmethod(fake)

    ctx = nx.GpuContext.__new__(nx.GpuContext)
    ctx._lib, ctx._h, ctx.compiled = Lib(), "h", fused._traj_ctx.compiled
    params = list(F)[::-1]
    values, length = ctx.traj_frame_values(t, moon, params, STEP)
    chain = eclipse.body_chain(nx.MOON, almanac, earth)
    assert [c[0] for c in calls] == [8, 8, 8, 1] and sum((c[1] for c in calls), []) == [int(p) for p in params]
    for c in calls:
        assert c[2:5] == (0, STEP, len(chain)) and list(zip(c[5], c[6])) == chain and c[7] == moon.mu_km3_s2
    assert values.shape == (25, 4, 3) and (length == 4).all() and (values[:, 0, 0] == [float(int(p)) for p in params]).all()
    calls.clear()
    ctx.traj_frame_values(t, earth, [nx.StateParameter.Rmag], STEP, EPOCH0_NS, EPOCH0_NS + STEP)
    assert calls == [(1, [int(F.Rmag)], 1, STEP, 0, [], [], earth.mu_km3_s2)]
    with pytest.raises(ValueError, match="at least one parameter"):
        ctx.traj_frame_values(t, moon, [], STEP)
    with pytest.raises(TypeError):
        ctx.traj_frame_values(t, moon, [nx.StateParameter.Cd], STEP)
    assert C.sizeof(_abi.FrameQuery) == 112
