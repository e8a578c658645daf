"""CPU: the one Python path of the five series reports (`Results._series` in nyx_amd/mc.py, `_param_series` in nyx_amd/propagator.py).

* The FUSED branch of `values_of`, `ric_dispersions`, `ground_tracks`, `station_views` and `eclipses`, with an injected evaluator that
  offers the fused entries in the entries' layout - NaN past `len`, a capacity larger than the longest series, for RIC `epoch0` and
  `moments[capacity, 28]` - built by composition from the host formulas: each report through it equals the report through the composing
  evaluator (no fused entry: the definition).  Five runs, one failed, one with a shorter trajectory, four samples at 60 s.
* `ground_tracks`, `station_views` and `eclipses` of a sharded ensemble (two gloo ranks, seven runs) equal the single-process result.
* The launcher with a recording callable in place of the ctypes entry: the launches, their queries, where they write."""
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
from nyx_amd import _abi, ephem, mc, propagator
from nyx_amd.eclipse import EclipseParameter as E, eclipse_value
from nyx_amd.groundtrack import GroundTrackParameter as G, ground_track_value
from nyx_amd.params import ric_difference, smooth_ric, state_value
from nyx_amd.stations import AerParameter as A, aer_value
from scenarios import EPOCH0_NS, leo_full_setup, leo_nominal
from test_ric_host import _free_port, assert_moments_within_the_summation_bound

S = nx.NS_PER_S
STEP = 60 * S
IAU_EARTH = nx.Frame(nx.EARTH, ephem.MU_EARTH, 6378.1363, nx.IAU_EARTH_ROTATION, 1.0 / 298.257)
STATIONS = [nx.GroundStation("Madrid", 40.427222, 4.250556, 0.834939, IAU_EARTH, 5.0),
            nx.GroundStation("Canberra", -35.398333, 148.981944, 0.691750, IAU_EARTH, 5.0)]
FAILED, SHORT = 3, 1
SPARE = 2                                                                      # slots of the entries' buffers past the longest series
WINDOWS = [(None, None), (EPOCH0_NS + STEP // 2, EPOCH0_NS + 3 * STEP)]        # the window: samples at 30, 90 and 150 s
FIELDS = ("values", "len", "epoch0_ns", "ok")


class Composing:
    """What Results needs from a context and no more: every report by composition."""

    traj_at = staticmethod(oracle_lib.traj_at)
    traj_every = staticmethod(oracle_lib.traj_every)

    def __init__(self, compiled):
        self.compiled, self.calls = compiled, 0


class Fused(Composing):
    """The five fused entries with GpuContext's signatures and layouts, composed from `traj_every` / `traj_at` and the host formulas.
    `calls` counts the launches: a report that quietly took the composition instead would compare the definition with itself."""

    def _series(self, tb, step, start_ns, end_ns, column, ref=None):
        """values[rows, capacity, n], len[n], lo[n], the columns: `column(rv[len, 6], epochs[len])` -> rows x [len] of every trajectory
        (against `ref`: `column(rv, rv of ref)` over the overlap)."""
        self.calls += 1
        lo, hi = propagator.series_bounds(tb, start_ns, end_ns) if ref is None else propagator.ric_bounds(tb, ref, start_ns, end_ns)
        live = np.nonzero(hi >= lo)[0]
        longest = int(((hi[live] - lo[live]) // step).max()) + 1 if len(live) else 1
        every = oracle_lib.traj_every(tb, step, longest) if start_ns is None and ref is None else None
        values, length, cols = None, np.zeros(tb.n, dtype=np.int32), []
        for i in live:
            q = lo[i] + step * np.arange((hi[i] - lo[i]) // step + 1, dtype=np.int64)
            if every is not None:
                rv = every.trajectory(i)[1]
            else:
                states, status = oracle_lib.traj_at(nx.Traj(None, tb, i)._single(), q)
                bad = _abi.interp_failed(status[:, 0])
                if ref is not None:
                    other, status = oracle_lib.traj_at(ref, q)
                    bad = bad | _abi.interp_failed(status[:, 0])
                end = np.nonzero(bad)[0]
                rv = states[: (end[0] if len(end) else len(q)), 0]
            cols.append(np.stack(column(rv, q[:len(rv)] if ref is None else other[:len(rv), 0])).reshape(-1, len(rv)))
            end = np.nonzero(np.isnan(cols[-1]).any(axis=0))[0]                  # (a sample that cannot be evaluated ends the series)
            cols[-1] = cols[-1][:, :int(end[0])] if len(end) else cols[-1]
            values = np.full((len(cols[-1]), longest + SPARE, tb.n), np.nan) if values is None else values
            length[i] = cols[-1].shape[1]
            values[:, :length[i], i] = cols[-1]
        return values, length, lo, cols

    def traj_values(self, tb, params, step_ns, start_ns=None, end_ns=None, mu_km3_s2=None):
        mu = float(self.compiled.central.mu_km3_s2 if mu_km3_s2 is None else mu_km3_s2)
        return self._series(tb, step_ns, start_ns, end_ns, lambda rv, ep: [state_value(p, rv, mu) for p in params])[:2]

    def traj_ground_track(self, tb, frame, params, step_ns, start_ns=None, end_ns=None):
        return self._series(tb, step_ns, start_ns, end_ns, lambda rv, ep: [ground_track_value(p, rv, ep, frame) for p in params])[:2]

    def traj_aer(self, tb, stations, params, step_ns, start_ns=None, end_ns=None):
        values, length = self._series(tb, step_ns, start_ns, end_ns, lambda rv, ep: [aer_value(p, rv, ep, st) for st in stations for p in params])[:2]
        return values.reshape(len(stations), len(params), *values.shape[1:]), length

    def traj_eclipse(self, tb, model, params, step_ns, start_ns=None, end_ns=None):
        pairs = [p if isinstance(p, tuple) else (p, None) for p in params]
        return self._series(tb, step_ns, start_ns, end_ns, lambda rv, ep: [eclipse_value(p, rv, ep, model, self.compiled.almanac, self.compiled.central, body=b)
                                                                           for p, b in pairs])[:2]

    def traj_ric_diff(self, tb, ref, step_ns, start_ns=None, end_ns=None, frame_of="reference", transport=True, smooth_window=5, moments=False):
        def column(a, b):
            d = ric_difference(a, b, frame_of=frame_of, transport=transport)
            return (smooth_ric(d, smooth_window) if smooth_window >= 3 else d).T

        values, length, lo, cols = self._series(tb, step_ns, start_ns, end_ns, column, ref)
        return values, length, np.where(length > 0, lo, 0), mc.ric_moments(cols, values.shape[1]) if moments else None


def _mc(evaluator, fail_index, opts=None):
    prop, almanac, central = leo_full_setup(degree=4, opts=opts)
    compiled = prop.compile(almanac, central)
    template = nx.Spacecraft(EPOCH0_NS, leo_nominal(), central, dry_mass_kg=100.0, prop_mass_kg=10.0, srp_area_m2=1.0, cr=1.8)
    mvn = nx.MvnSpacecraft.from_sigmas(template, [1.0, 1.0, 1.0, 1e-3, 1e-3, 1e-3])

    def fn(batch, end_epoch_ns):
        out, st, traj = oracle_lib.propagate_with_traj(compiled, batch, end_epoch_ns - int(batch.epoch_ns[0]), 256)
        if fail_index is not None:
            st.status[fail_index] = _abi.ERR_NAN
        return out, st, traj, evaluator(compiled)

    return prop, almanac, compiled, template, nx.MonteCarlo(mvn, seed=3, propagate_fn=fn)


@pytest.fixture(scope="module")
def world():
    """(results through the fused evaluator, the same results through the composing one, nominal, shadow model)."""
    prop, almanac, compiled, template, carlo = _mc(Fused, FAILED, nx.IntegratorOptions.with_fixed_step(20 * S))   # ten stored states in 180 s
    fused = carlo.run_until_epoch(prop, almanac, EPOCH0_NS + 3 * STEP, 5)
    tb, row = fused._traj_batch, fused._traj_rows[fused.runs[SHORT].index]
    keep = int(np.searchsorted(tb.epoch_ns[: tb.len[row], row], EPOCH0_NS + 2 * STEP + 1))    # run SHORT ends between samples 2 and 3
    assert 2 < keep < tb.len[row]
    tb.len[row] = keep
    nominal = oracle_lib.propagate_with_traj(compiled, nx.pack_spacecraft([template], False), 3 * STEP, 256)[2]
    return fused, dataclasses.replace(fused, _traj_ctx=Composing(compiled)), nominal, nx.ShadowModel.cislunar(almanac)


REPORTS = {"values": lambda r, w, win: r.values_of([nx.StateParameter.X, nx.StateParameter.Cr, nx.StateParameter.Rmag, nx.StateParameter.PropMass], STEP, *win),
           "values_filled": lambda r, w, win: r.values_of([nx.StateParameter.SemiMajorAxis], STEP, *win, value_if_run_failed=-7.0),
           "values_of_the_host_only": lambda r, w, win: r.values_of([nx.StateParameter.Cd, nx.StateParameter.DryMass], STEP, *win),
           "ric": lambda r, w, win: r.ric_dispersions(w[2], STEP, *win),
           "ric_own_frame": lambda r, w, win: r.ric_dispersions(w[2], STEP, *win, frame_of="run", transport=False, smooth_window=3),
           "ground_tracks": lambda r, w, win: r.ground_tracks(IAU_EARTH, STEP, [G.Latitude, G.Longitude, G.Height], *win),
           "station_views": lambda r, w, win: r.station_views(STATIONS, STEP, [A.Azimuth, A.Elevation, A.Range], *win),
           "eclipses": lambda r, w, win: r.eclipses(w[3], STEP, [E.Occultation, E.State, (E.BodyOccultation, 0)], *win)}


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("report", REPORTS)
def test_the_fused_branch_equals_the_composition(world, report, window):
    fused, composed = world[:2]
    fused._traj_ctx.calls = composed._traj_ctx.calls = 0
    a = REPORTS[report](fused, world, window)
    assert fused._traj_ctx.calls == 1 and composed._traj_ctx.calls == 0         # one launch ...
    b = REPORTS[report](composed, world, window)
    assert type(a) is type(b) and dataclasses.fields(a) == dataclasses.fields(b) and a.step_ns == b.step_ns == STEP
    for f in FIELDS + (("count",) if report.startswith("ric") else ()):         # ... and the same series, bit for bit
        assert getattr(a, f).dtype == getattr(b, f).dtype
        np.testing.assert_array_equal(getattr(a, f), getattr(b, f))
    assert list(a.len) == ([4, 3, 4, 0, 4] if window[0] is None else [3, 2, 3, 0, 3]) and list(a.ok) == [j != FAILED for j in range(5)]
    assert a.values.shape[-2:] == (a.len.max(), 5) and np.isfinite(a.values[..., :a.len[SHORT], SHORT]).all()
    if report.startswith("ric"):                                                # the sums: the tolerances of tests/test_ric_host.py
        assert a.moments.shape == b.moments.shape == (a.len.max(), _abi.RIC_MOMENTS)
        for k in range(len(a.moments)):
            have = [j for j in range(5) if k < a.len[j]]
            assert_moments_within_the_summation_bound(a.moments[k], a.values[:, k, have].T)
            assert_moments_within_the_summation_bound(b.moments[k], a.values[:, k, have].T)
        np.testing.assert_allclose(a.mean, b.mean, rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(a.cov, b.cov, rtol=1e-9, atol=1e-12 * np.nanmax(np.abs(b.cov)))
    elif report == "station_views":
        np.testing.assert_array_equal(a.of(STATIONS[1], A.Range), b.values[1, 2])


# ---- a sharded ensemble ----------------------------------------------------------------------------------------------
SHARDED = ("ground_tracks", "station_views", "eclipses")
END = EPOCH0_NS + 5 * STEP


def _sharded_reports(res, almanac):
    w = (None, None, None, nx.ShadowModel.cislunar(almanac))
    return {(name, k): REPORTS[name](res, w, win) for name in SHARDED for k, win in enumerate([(None, None), (EPOCH0_NS + 100 * S, EPOCH0_NS + 250 * S)])}


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    prop, almanac, _, _, carlo = _mc(Composing, 1)          # position 1 of EVERY shard fails: runs 1 and 5 of 7
    res = carlo.resume_run_until_epoch(prop, almanac, 0, END, 7, dist=dist)
    got = {f"{name}{k}_{f}": getattr(series, f) for (name, k), series in _sharded_reports(res, almanac).items() for f in FIELDS}
    outcome = "no error"
    try:
        res.station_views(STATIONS if rank == 0 else [], STEP)                 # one rank refuses: both raise, neither waits in a collective
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
    for (name, k), series in _sharded_reports(res, almanac).items():
        assert list(series.len) == [0 if j in (1, 5) else (3 if k else 6) for j in range(7)] and series.values.shape[-2:] == ((3 if k else 6), 7)
        for f in FIELDS:
            for rank in range(2):                                              # every rank holds the complete result (NaN == NaN here)
                got = v[rank][f"{name}{k}_{f}"]
                assert got.dtype == getattr(series, f).dtype
                np.testing.assert_array_equal(got, getattr(series, f), err_msg=f"{name} {k} {f} on rank {rank}")


# ---- the launcher ----------------------------------------------------------------------------------------------------
def _value(group, code, k, i):
    return 1000.0 * group + 10.0 * code + 0.1 * k + 0.001 * i


@pytest.mark.parametrize("n_groups,n_codes,want", [(None, 9, [(None, 8), (None, 1)]), (17, 9, [(16, 8), (16, 1), (1, 8), (1, 1)]), (17, 5, [(16, 5), (1, 5)])])
@pytest.mark.parametrize("window", [(None, None), (EPOCH0_NS + 30 * S, EPOCH0_NS + 170 * S)])
def test_param_series_launches(n_groups, n_codes, want, window):
    t = _abi.TrajBatch(3, 4)
    t.len[:] = 4
    t.epoch_ns[:] = (EPOCH0_NS + STEP * np.arange(4, dtype=np.int64))[:, None]
    cap = 4 if window[0] is None else 3
    codes, calls, filled = list(range(20, 20 + n_codes)), [], []

    def fake(handle, ctraj, n, q, capacity, values, length):
        q = q._obj
        assert handle == "h" and n == 3 and capacity == cap
        g, p = getattr(q, "n_stations", None), list(q.param[:q.n_params])
        calls.append(((g if n_groups else None), q.n_params, p, q.has_window, q.step_ns, q.start_ns, q.end_ns, C.addressof(values.contents)))
        base = int(q.stations[0].latitude_deg) if n_groups else 0               # the first group of this launch, as fill_group named it
        out = np.ctypeslib.as_array(values, shape=(g if n_groups else 1, q.n_params, capacity, n))
        for s, c, k, i in np.ndindex(*out.shape):
            out[s, c, k, i] = _value(base + s, p[c], k, i)
        np.ctypeslib.as_array(length, shape=(n,))[:] = capacity
        return 0

    def fill_group(q, group):
        q.n_stations, q.stations[0].latitude_deg = len(group), group[0]

    groups = (list(range(n_groups)), _abi.MAX_STATIONS, fill_group) if n_groups else None
    values, length = propagator._param_series("traj_x", fake, "h", _abi.AerQuery, 8, filled.append, t, codes, STEP, *window, None, groups)
    assert values.shape == ((n_groups,) if n_groups else ()) + (n_codes, cap, 3) and (length == cap).all() and len(filled) == len(calls)
    assert [c[:2] for c in calls] == want
    lo = 0
    for c in calls:                                                            # the parameters of a group in order, then the next group
        assert c[2] == codes[lo:lo + c[1]] and c[3:7] == ((0, STEP, 0, 0) if window[0] is None else (1, STEP) + window)
        lo = (lo + c[1]) % n_codes
    for idx in np.ndindex(*values.shape):
        assert values[idx] == _value(*(((0,) if not n_groups else ()) + idx[:-3]), codes[idx[-3]], idx[-2], idx[-1])
    # a launch that fills a contiguous block of the result writes there, one that covers part of the parameters of a group does not
    if not n_groups or n_codes <= 8:
        assert [c[7] for c in calls] == [values.ctypes.data, values[8 if not n_groups else 16:].ctypes.data]
    else:
        assert values.ctypes.data not in [c[7] for c in calls]


def test_param_series_refusals():
    t = _abi.TrajBatch(1, 2)
    with pytest.raises(ValueError, match="traj_x: a window needs both start_ns and end_ns"):
        propagator._param_series("traj_x", None, None, _abi.GtQuery, 8, None, t, [1], STEP, EPOCH0_NS, None, None)
    with pytest.raises(RuntimeError, match=r"nyx_hip_traj_x failed \(rc=-3\)"):
        propagator._param_series("traj_x", lambda *a: -3, None, _abi.GtQuery, 8, lambda q: None, t, [1], STEP, None, None, 2)
