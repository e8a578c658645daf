"""CPU: the link report through the one Python path of the series reports (`Results._series` in nyx_amd/mc.py, `_param_series` in
nyx_amd/propagator.py), the pattern of tests/test_frame_one_path.py and its injected evaluators.

* The FUSED branch of `Results.link_views`, with an evaluator that offers `traj_link` in the entry's layout - NaN past `len`, a
  capacity larger than the longest series, the rows of failed runs emptied by the caller - built by composition from
  `links.link_value`: it equals the report through the composing evaluator (no fused entry: the definition) bit for bit, with ONE
  launch counted.  Five runs, one failed, one with a shorter trajectory, both windows; the transmitter is the nominal flown
  retrograde, the bodies the Earth and the Moon.
* The default bodies (None: the centre), and a transmitter whose span is shorter than the runs'.
* `LinkSeries.visible_fraction` / `closest_range` against numpy on the columns; `Traj.link_view` against the same launch.
* The launcher: more than eight parameters split into launches; the bodies, `param_body`, the second batch and the first epochs in
  every call; the existing entries called exactly as before."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import nyx_amd as nx
import oracle_lib
from nyx_amd import _abi, eclipse, links, propagator
from nyx_amd.links import LinkParameter as L
from scenarios import EPOCH0_NS, leo_nominal
from test_series_one_path import FAILED, FIELDS, SHORT, SPARE, STEP, WINDOWS, Composing, _mc

S = nx.NS_PER_S
PARAMS = [L.Range, L.RangeRate, L.Visible, L.Clearance, (L.BodyClearance, 1), (L.BodyObstructs, 0)]


class Fused(Composing):
    """`traj_link` with GpuContext's signature and layout, composed from `traj_at` and the host definition.  `calls` counts the
    launches: a report that quietly took the composition instead would compare the definition with itself."""

    def traj_link(self, tb, ref, params, step_ns, start_ns=None, end_ns=None, capacity=None, bodies=None):
        self.calls += 1
        al, central = self.compiled.almanac, self.compiled.central
        who = links.default_bodies(central) if bodies is None else list(bodies)
        pairs = [links.link_param(p, who) for p in params]
        lo, hi = propagator.ric_bounds(tb, ref, start_ns, end_ns)
        live = np.nonzero(hi >= lo)[0]
        longest = int(((hi[live] - lo[live]) // step_ns).max()) + 1 if len(live) else 1
        values, length = np.full((len(params), longest + SPARE, tb.n), np.nan), np.zeros(tb.n, dtype=np.int32)
        for i in live:
            q = lo[i] + step_ns * np.arange((hi[i] - lo[i]) // step_ns + 1, dtype=np.int64)
            rx, sa = oracle_lib.traj_at(nx.Traj(None, tb, i)._single(), q)
            tx, sb = oracle_lib.traj_at(ref if ref.n == 1 else nx.Traj(None, ref, i)._single(), q)
            end = np.nonzero(_abi.interp_failed(sa[:, 0]) | _abi.interp_failed(sb[:, 0]) | links.outside_ephemerides(q, who, al, central))[0]
            k = int(end[0]) if len(end) else len(q)
            length[i] = k
            values[:, :k, i] = np.stack([links.link_value(p, rx[:k, 0], tx[:k, 0], q[:k], who, al, central, body=b) for p, b in pairs]).reshape(len(pairs), k)
        return values, length, np.where(hi >= lo, lo, 0)


@pytest.fixture(scope="module")
def world():
    """(results through the fused evaluator, the same through the composing one, the transmitter, a shorter one, the bodies)."""
    prop, almanac, compiled, template, carlo = _mc(Fused, FAILED, nx.IntegratorOptions.with_fixed_step(20 * S))   # ten stored states in 180 s
    fused = carlo.run_until_epoch(prop, almanac, EPOCH0_NS + 3 * STEP, 5)
    tb, row = fused._traj_batch, fused._traj_rows[fused.runs[SHORT].index]
    keep = int(np.searchsorted(tb.epoch_ns[: tb.len[row], row], EPOCH0_NS + 2 * STEP + 1))    # run SHORT ends between samples 2 and 3
    assert 2 < keep < tb.len[row]
    tb.len[row] = keep
    batch = nx.pack_spacecraft([template], False)
    batch.set_rv((leo_nominal() * np.array([1.0, 1.0, 1.0, -1.0, -1.0, -1.0]))[None, :])
    tx = oracle_lib.propagate_with_traj(compiled, batch, 3 * STEP, 256)[2]
    short = oracle_lib.propagate_with_traj(compiled, batch, STEP + STEP // 2, 256)[2]
    return fused, dataclasses.replace(fused, _traj_ctx=Composing(compiled)), tx, short, [compiled.central, almanac.frame_info(nx.MOON)]


@pytest.mark.parametrize("window", WINDOWS)
def test_the_fused_branch_equals_the_composition(world, window):
    fused, composed, tx, _, bodies = world
    fused._traj_ctx.calls = composed._traj_ctx.calls = 0
    a = fused.link_views(tx, STEP, PARAMS, bodies, *window)
    assert fused._traj_ctx.calls == 1 and composed._traj_ctx.calls == 0         # one launch ...
    b = composed.link_views(tx, STEP, PARAMS, bodies, *window)
    assert type(a) is type(b) is nx.LinkSeries and dataclasses.fields(a) == dataclasses.fields(b) and a.step_ns == b.step_ns == STEP
    for f in FIELDS:                                                            # ... and the same series, bit for bit
        assert getattr(a, f).dtype == getattr(b, f).dtype
        np.testing.assert_array_equal(getattr(a, f), getattr(b, f))
    assert a.params == PARAMS and a.bodies == bodies
    assert list(a.len) == ([4, 3, 4, 0, 4] if window[0] is None else [3, 2, 3, 0, 3]) and list(a.ok) == [j != FAILED for j in range(5)]
    assert a.values.shape == (len(PARAMS), a.len.max(), 5) and np.isfinite(a.values[:, :a.len[SHORT], SHORT]).all()
    assert np.isnan(a.values[:, a.len[SHORT]:, SHORT]).all() and np.isnan(a.values[:, :, FAILED]).all()
    first = EPOCH0_NS if window[0] is None else window[0]
    assert [int(e) for e in a.epoch0_ns] == [0 if j == FAILED else first for j in range(5)]
    np.testing.assert_array_equal(a.epochs(0), first + STEP * np.arange(a.len[0]))
    # the two start at one place and fly apart, head-on: the range grows from a few km, the Moon is far from the line
    held = np.arange(a.values.shape[1])[:, None] < a.len[None, :]
    rng_km = a.of(L.Range)
    if window[0] is None:
        assert (rng_km[0][a.ok] < 10.0).all()
    assert (np.diff(rng_km[:, 0][:a.len[0]]) > 0).all() and (a.of(L.RangeRate)[held & (rng_km > 100.0)] > 15.0).all()
    assert (a.of((L.BodyClearance, 1))[held] > 3e5).all()
    np.testing.assert_array_equal(a.of(L.Visible)[held], 1.0 - a.of((L.BodyObstructs, 0))[held])
    # the helpers against numpy on the columns
    frac = a.visible_fraction()
    for k in range(a.values.shape[1]):
        has = [j for j in range(5) if k < a.len[j]]
        assert frac[k] == np.mean([a.of(L.Visible)[k, j] for j in has])
    best, when = a.closest_range()
    for j in range(5):
        col = rng_km[:a.len[j], j]
        assert (best[j], when[j]) == (col.min(), first + STEP * int(np.argmin(col))) if a.len[j] else (np.isnan(best[j]) and when[j] == 0)
    with pytest.raises(ValueError, match="does not hold Range"):
        fused.link_views(tx, STEP, [L.Visible], None, *window).closest_range()
    with pytest.raises(ValueError, match="holds none of"):
        fused.link_views(tx, STEP, [L.Range], None, *window).visible_fraction()
    # the visible share from what else tells
    for p in (L.ObstructingBody, L.Clearance):
        np.testing.assert_array_equal(fused.link_views(tx, STEP, [p], bodies, *window).visible_fraction(), frac)


@pytest.mark.parametrize("window", WINDOWS)
def test_the_default_bodies_and_a_shorter_transmitter(world, window):
    fused, composed, tx, short, bodies = world
    fused._traj_ctx.calls = 0
    a = fused.link_views(short, STEP, start_ns=window[0], end_ns=window[1])
    b = composed.link_views(short, STEP, start_ns=window[0], end_ns=window[1])
    assert fused._traj_ctx.calls == 1
    for f in FIELDS:
        np.testing.assert_array_equal(getattr(a, f), getattr(b, f))
    assert a.params == list(links.DEFAULT_PARAMS) and [int(x.naif_id) for x in a.bodies] == [nx.EARTH]
    # the transmitter ends after 90 s: samples at 0 and 60 s, or at 30 and 90 s in the window
    assert list(a.len) == [0 if j == FAILED else 2 for j in range(5)]
    # the same answer as with the centre named, and as the Traj of the transmitter gives
    c = fused.link_views(nx.Traj(None, short, 0), STEP, links.DEFAULT_PARAMS, [bodies[0]], *window)
    for f in FIELDS:
        np.testing.assert_array_equal(getattr(a, f), getattr(c, f))


def test_traj_link_view_is_the_same_launch(world):
    fused, _, tx, _, bodies = world
    ctx = fused._traj_ctx
    run = nx.Traj(ctx, fused._traj_batch, fused._traj_rows[fused.runs[0].index])
    ep, vals = run.link_view(nx.Traj(ctx, tx, 0), STEP, [L.Range, (L.BodyClearance, 1)], bodies=bodies)
    series = fused.link_views(tx, STEP, [L.Range, (L.BodyClearance, 1)], bodies)
    np.testing.assert_array_equal(ep, series.epochs(0))
    np.testing.assert_array_equal(vals, series.values[:, :series.len[0], 0])
    ep, vals = run.link_view(nx.Traj(ctx, tx, 0), STEP)
    assert vals.shape == (3, 4) and len(ep) == 4


# ---- the launcher ----------------------------------------------------------------------------------------------------
def test_more_than_eight_parameters_split_into_launches(world):
    """`GpuContext.traj_link` through `_param_series` with a recording callable in place of the ctypes entry."""
    fused, _, _, _, bodies = world
    almanac, earth = fused._traj_ctx.compiled.almanac, fused._traj_ctx.compiled.central
    t = _abi.TrajBatch(3, 4)
    t.len[:] = 4
    t.epoch_ns[:] = (EPOCH0_NS + STEP * np.arange(4, dtype=np.int64))[:, None]
    ref = _abi.TrajBatch(1, 3)
    ref.len[:] = 3
    ref.epoch_ns[:, 0] = EPOCH0_NS + STEP * np.arange(3, dtype=np.int64)
    calls = []

    def fake(handle, ctraj, n, cref, n_ref, q, capacity, values, length, epoch0):
        q = q._obj
        calls.append((q.n_params, list(q.param[:q.n_params]), list(q.param_body[:q.n_params]), q.has_window, q.step_ns, q.n_bodies,
                      [(b.n_chain, list(zip(b.chain_segment[:b.n_chain], b.chain_sign[:b.n_chain])), b.mean_radius_km) for b in q.bodies[:q.n_bodies]],
                      n, n_ref, capacity, cref._obj.capacity))
        out = np.ctypeslib.as_array(values, shape=(q.n_params, capacity, n))
        for c in range(q.n_params):
            out[c] = float(q.param[c]) + 0.5 * q.param_body[c]
        np.ctypeslib.as_array(length, shape=(n,))[:] = capacity
        np.ctypeslib.as_array(epoch0, shape=(n,))[:] = 77
        return 0

    class Lib:
        nyx_hip_traj_link = staticmethod(fake)

    ctx = nx.GpuContext.__new__(nx.GpuContext)
    ctx._lib, ctx._h, ctx.compiled = Lib(), "h", fused._traj_ctx.compiled
    params = [p for p in L if p not in links.PER_BODY] + [(L.BodyClearance, 0), (L.BodyClearance, bodies[1]), (L.BodyObstructs, 1)]
    values, length, epoch0 = ctx.traj_link(t, ref, params, STEP, bodies=bodies)
    chain = eclipse.body_chain(nx.MOON, almanac, earth)
    assert [c[0] for c in calls] == [8, 5] and sum((c[1] for c in calls), []) == list(range(10)) + [10, 10, 11]
    assert sum((c[2] for c in calls), []) == [0] * 10 + [0, 1, 1]
    for c in calls:
        assert c[3:6] == (0, STEP, 2) and c[6] == [(0, [], earth.mean_equatorial_radius_km), (len(chain), chain, bodies[1].mean_equatorial_radius_km)]
        assert c[7:] == (3, 1, 3, 3)                                         # the overlap sizes the series: three samples; the second batch went along
    assert values.shape == (13, 3, 3) and (length == 3).all() and (epoch0 == 77).all()
    assert list(values[:, 0, 0]) == [float(k) for k in range(10)] + [10.0, 10.5, 11.5]
    calls.clear()
    # the default: the centre alone, no segment named; a window; a capacity of the caller's
    ctx.traj_link(t, ref, [L.Visible], STEP, EPOCH0_NS, EPOCH0_NS + STEP, capacity=9)
    assert calls == [(1, [int(L.Visible)], [0], 1, STEP, 1, [(0, [], earth.mean_equatorial_radius_km)], 3, 1, 9, 3)]
    calls.clear()
    ctx.traj_link(t, ref, [L.Range], STEP, bodies=[])
    assert calls[0][5:7] == (0, [])
    with pytest.raises(ValueError, match="at least one parameter"):
        ctx.traj_link(t, ref, [], STEP)
    with pytest.raises(TypeError):
        ctx.traj_link(t, ref, [nx.StateParameter.Rmag], STEP)
    with pytest.raises(ValueError, match="names no body"):
        ctx.traj_link(t, ref, [(L.BodyClearance, 0)], STEP, bodies=[])
    with pytest.raises(ValueError, match="a window needs both"):
        ctx.traj_link(t, ref, [L.Range], STEP, start_ns=5)
    with pytest.raises(ValueError, match="one, or one per run"):
        ctx.traj_link(t, _abi.TrajBatch(2, 3), [L.Range], STEP)
    assert C.sizeof(_abi.LinkQuery) == 488


def test_the_existing_entries_are_called_as_before(world):
    """`_param_series` without the new arguments: seven arguments, nothing behind `len`."""
    fused = world[0]
    t = _abi.TrajBatch(2, 4)
    t.len[:] = 4
    t.epoch_ns[:] = (EPOCH0_NS + STEP * np.arange(4, dtype=np.int64))[:, None]
    seen = []

    def fake(*args):
        seen.append(len(args))
        np.ctypeslib.as_array(args[5], shape=(args[3]._obj.n_params, args[4], args[2]))[:] = 1.0
        return 0

    class Lib:
        nyx_hip_traj_values = staticmethod(fake)

    ctx = nx.GpuContext.__new__(nx.GpuContext)
    ctx._lib, ctx._h, ctx.compiled = Lib(), "h", fused._traj_ctx.compiled
    values, length = ctx.traj_values(t, [nx.StateParameter.Rmag], STEP)
    assert seen == [7] and values.shape == (1, 4, 2) and (values == 1.0).all()
