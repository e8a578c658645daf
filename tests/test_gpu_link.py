"""The link report on the MI355X (link_kernel.hip, include/nyx_hip_link.h).

The two inertial states a value is evaluated from are the ones `traj_every` / `traj_at` return (same device code), and the
ephemerides, the SIGHT test and the parameters are the code tests/test_link_host_cxx.py runs on the CPU against the host definition:
the values are compared with `nyx_amd.links.link_value` applied to those states at their epochs.  Small on purpose: at most 70
trajectories, one orbit.

THE ENSEMBLE is the family's fixture: `leo_full_setup(degree=8)`, `dispersed_leo_batch(70, seed=11)`, 5400 s, dense capacity 256,
step 60 s, 91 samples - one full wave plus one with 6 live lanes.  THE TRANSMITTER is the nominal with its velocity reversed,
(r, -v): the same orbit flown retrograde.  With two-body motion that gives 74 of 91 samples obstructed by the Earth, four transitions
(after samples 3, 40, 50 and 87) and a smallest |clearance| at a sample of 4.5 km; the fixture asserts on the host definition applied
to the `traj_every` states that the obstructed share lies in [0.5, 0.95] and that every run has at least two transitions - otherwise
the Visible cases would test nothing.

THE BOUND IS ZERO for all twelve parameters: every one is formed with + - * / sqrt and comparisons only, each a correctly rounded
IEEE operation on both sides, in one order (csrc/link_dev.h restates nyx_amd/links.py operation for operation, compiled with
-ffp-contract=off).  Bits are compared; NaN must stand where the definition has NaN, and nowhere else."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import nyx_amd as nx
from nyx_amd import _abi, eclipse, links
from nyx_amd.links import LinkParameter as L
from scenarios import EPOCH0_NS, dispersed_leo_batch, leo_full_setup, leo_nominal

pytestmark = pytest.mark.gpu

S = nx.NS_PER_S
STEP = 60 * S
DUR = 5400 * S
COUNT = 91
TILE = 4           # LNK_TILE of csrc/link_kernel.hip
RETRO = np.array([1.0, 1.0, 1.0, -1.0, -1.0, -1.0])
WHOLE = [p for p in L if p not in links.PER_BODY]
ALL = WHOLE + [(L.BodyClearance, 0), (L.BodyClearance, 1), (L.BodyObstructs, 0), (L.BodyObstructs, 1)]    # fourteen rows: two launches


def row(p):
    return ALL.index(p)


def same_bits(got, want, label=""):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (label, got.shape, want.shape)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=f"{label}: NaN pattern")
    held = ~np.isnan(want)
    bad = got[held].view(np.uint64) != want[held].view(np.uint64)
    worst = float(np.abs(got[held] - want[held])[np.isfinite(want[held])].max()) if held.any() and np.isfinite(want[held]).any() else 0.0
    print(f"deviation {label:28s} {worst:.3e}  (bound 0, {int(held.sum())} values, {int(bad.sum())} differ in bits)")
    assert not bad.any(), f"{label}: {int(bad.sum())} of {int(held.sum())} values differ, the largest by {worst:.3e}"


def host_values(world, params, rx, tx, epochs, bodies):
    """[P, ...] of the host definition; params as LinkParameter or (per-body LinkParameter, index)."""
    pairs = [p if isinstance(p, tuple) else (p, None) for p in params]
    return np.stack([links.link_value(p, rx, tx, epochs, bodies, world["almanac"], world["central"], body=b) for p, b in pairs])


@pytest.fixture(scope="module")
def world():
    prop, almanac, central = leo_full_setup(degree=8)
    compiled = prop.compile(almanac, central)
    ctx = nx.GpuContext(compiled)
    yield dict(prop=prop, almanac=almanac, central=central, compiled=compiled, ctx=ctx, moon=almanac.frame_info(nx.MOON),
               both=[central, almanac.frame_info(nx.MOON)])
    ctx.close()


def retrograde(batch):
    out = batch.copy()
    out.set_rv(batch.rv() * RETRO[None, :])
    return out


@pytest.fixture(scope="module")
def leo70(world):
    """One orbit of 70 dispersed receivers and of the retrograde transmitter with dense output, their traj_every states, the host
    definition on those states and the device's values at capacity 91: computed once, shared, never written to."""
    ctx = world["ctx"]
    _, st, traj = ctx.propagate_with_traj(dispersed_leo_batch(70, seed=11), DUR, capacity=256)
    assert (st.status == 0).all()
    nominal = dispersed_leo_batch(1, seed=0)
    nominal.set_rv(leo_nominal()[None, :])
    _, st, tx = ctx.propagate_with_traj(retrograde(nominal), DUR, capacity=256)
    assert (st.status == 0).all() and tx.n == 1
    ev, evt = ctx.traj_every(traj, STEP, COUNT), ctx.traj_every(tx, STEP, COUNT)
    assert (ev.len == COUNT).all() and (evt.len == COUNT).all()
    rx = np.ascontiguousarray(ev.state.transpose(1, 2, 0))               # [K, n, 6]
    txs = np.ascontiguousarray(evt.state.transpose(1, 2, 0))             # [K, 1, 6]
    want = host_values(world, ALL, rx, txs, ev.epoch_ns, world["both"])  # [14, K, n]
    hidden = want[row(L.Visible)] == 0.0
    assert 0.5 <= hidden.mean() <= 0.95, hidden.mean()
    assert ((np.diff(hidden.astype(np.int8), axis=0) != 0).sum(axis=0) >= 2).all()
    print(f"obstructed share {hidden.mean():.3f}; smallest |clearance| {np.abs(want[row(L.Clearance)]).min():.2f} km")
    got, length, epoch0 = ctx.traj_link(traj, tx, ALL, STEP, capacity=COUNT, bodies=world["both"])
    for a in (ev.state, ev.epoch_ns, rx, txs, want, got, length, epoch0):
        a.setflags(write=False)
    return dict(traj=traj, tx=tx, ev=ev, evt=evt, rx=rx, txs=txs, want=want, got=got, len=length, epoch0=epoch0)


def head(traj, cols):
    """The trajectories `cols` of a batch as a batch of their own."""
    cols = list(range(cols)) if isinstance(cols, int) else list(cols)
    t = _abi.TrajBatch(len(cols), traj.capacity)
    t.epoch_ns[:], t.state[:], t.len[:] = traj.epoch_ns[:, cols], traj.state[:, :, cols], traj.len[cols]
    return t


def link_query(world, params, bodies, step=STEP, start=None, stop=None):
    """The query GpuContext.traj_link builds, for the raw entries."""
    q = _abi.LinkQuery()
    q.n_params, q.step_ns, q.n_bodies = len(params), step, len(bodies)
    for k, p in enumerate(params):
        p, b = links.link_param(p, bodies)
        q.param[k], q.param_body[k] = int(p), b
    if start is not None:
        q.has_window, q.start_ns, q.end_ns = 1, start, stop
    for b, frame in enumerate(bodies):
        chain = links.link_chain(frame, world["almanac"], world["central"])
        q.bodies[b].n_chain, q.bodies[b].mean_radius_km = len(chain), float(frame.mean_equatorial_radius_km)
        for k, (seg, sign) in enumerate(chain):
            q.bodies[b].chain_segment[k], q.bodies[b].chain_sign[k] = seg, sign
    return q


def test_1_all_twelve_parameters_against_the_earth_and_the_moon(world, leo70):
    got, want, length = leo70["got"], leo70["want"], leo70["len"]
    assert len(WHOLE) == 10 and {int(p if not isinstance(p, tuple) else p[0]) for p in ALL} == set(range(12))
    assert got.shape == (14, COUNT, 70) and length.dtype == np.int32 and (length == COUNT).all() and (leo70["epoch0"] == EPOCH0_NS).all()
    for j, p in enumerate(ALL):
        same_bits(got[j], want[j], p.name if not isinstance(p, tuple) else f"{p[0].name}[{p[1]}]")
    assert np.isfinite(got).all()
    # the Moon never obstructs and is where it is
    moon = got[row((L.BodyClearance, 1))]
    assert (got[row((L.BodyObstructs, 1))] == 0.0).all() and (moon > 3e5).all() and (moon < 4.2e5).all()
    # the figures hang together on the device's own values
    np.testing.assert_array_equal(got[row(L.Clearance)], np.minimum(got[row((L.BodyClearance, 0))], moon))
    np.testing.assert_array_equal(got[row(L.Visible)], 1.0 - np.maximum(got[row((L.BodyObstructs, 0))], got[row((L.BodyObstructs, 1))]))
    first = got[row(L.ObstructingBody)]
    assert ((first == 0.0) | (first == -1.0)).all() and ((first == 0.0) == (got[row(L.Visible)] == 0.0)).all()
    assert ((got[row((L.BodyClearance, 0))] <= 0.0) == (got[row((L.BodyObstructs, 0))] == 1.0)).all()
    with pytest.raises(TypeError):
        world["ctx"].traj_link(leo70["traj"], leo70["tx"], [L.Range, nx.AerParameter.Range], STEP)
    with pytest.raises(KeyError, match="planetary data"):
        world["ctx"].traj_link(leo70["traj"], leo70["tx"], [L.Visible], STEP, bodies=[nx.Frame(499, 42828.0, 3396.0)])


def test_2_one_transmitter_per_run(world, leo70):
    """70 dispersed retrograde transmitters, all built from one nominal: the pairwise result is, lane by lane, the result of a call
    with that one transmitter on that one run - lanes 0, 63 and 64."""
    ctx = world["ctx"]
    traj = leo70["traj"]
    _, st, txs = ctx.propagate_with_traj(retrograde(dispersed_leo_batch(70, seed=12)), DUR, capacity=256)
    assert (st.status == 0).all()
    params = [L.Range, L.RangeRate, L.ReferenceDoppler, L.Visible, L.Clearance, L.LosZ, (L.BodyClearance, 1), (L.BodyObstructs, 0)]
    got, length, epoch0 = ctx.traj_link(traj, txs, params, STEP, capacity=COUNT, bodies=world["both"])
    assert (length == COUNT).all() and np.isfinite(got).all()
    for lane in (0, 63, 64):
        one, l1, e1 = ctx.traj_link(head(traj, [lane]), head(txs, [lane]), params, STEP, capacity=COUNT, bodies=world["both"])
        assert l1[0] == COUNT and e1[0] == epoch0[lane]
        same_bits(got[:, :, lane], one[:, :, 0], f"pairwise lane {lane}")
    # and it is the definition on the traj_every states of both batches
    ev, evt = leo70["ev"], ctx.traj_every(txs, STEP, COUNT)
    want = host_values(world, params, leo70["rx"], np.ascontiguousarray(evt.state.transpose(1, 2, 0)), ev.epoch_ns, world["both"])
    same_bits(got, want, "pairwise against the definition")
    assert not np.array_equal(got[0], leo70["got"][row(L.Range)])             # (they are other transmitters)


def test_3_spans(world, leo70):
    ctx = world["ctx"]
    traj, tx, full = leo70["traj"], leo70["tx"], leo70["got"]
    params = [L.Range, L.Visible, L.Clearance]
    rows = [row(p) for p in params]
    both = world["both"]
    # a transmitter propagated for 3000 s only: the series ends with it
    nominal = dispersed_leo_batch(1, seed=0)
    nominal.set_rv(leo_nominal()[None, :])
    _, st, short = ctx.propagate_with_traj(retrograde(nominal), 3000 * S, capacity=256)
    got, length, epoch0 = ctx.traj_link(traj, short, params, STEP, bodies=both)      # capacity=None: sized from the two batches
    assert got.shape == (3, 51, 70) and (length == 51).all() and (epoch0 == EPOCH0_NS).all()
    ev, evt = ctx.traj_every(traj, STEP, 51), ctx.traj_every(short, STEP, 51)
    want = host_values(world, params, ev.state.transpose(1, 2, 0), evt.state.transpose(1, 2, 0), ev.epoch_ns, both)
    same_bits(got, want, "short transmitter")
    # a window inside the overlap that starts at sample 7: the slice of the full series, bit for bit
    start, stop = EPOCH0_NS + 7 * STEP, EPOCH0_NS + 40 * STEP + 5 * S
    got, length, epoch0 = ctx.traj_link(traj, tx, params, STEP, start, stop, bodies=both)
    assert got.shape == (3, 34, 70) and (length == 34).all() and (epoch0 == start).all()
    same_bits(got, full[rows, 7:41], "window")
    # a window outside the overlap: nothing, all NaN
    got, length, epoch0 = ctx.traj_link(traj, tx, params, STEP, EPOCH0_NS + DUR + S, EPOCH0_NS + DUR + 500 * S, capacity=5, bodies=both)
    assert (length == 0).all() and np.isnan(got).all() and got.shape == (3, 5, 70) and (epoch0 == 0).all()
    # a capacity smaller than the series: counted, not stored
    got, length, _ = ctx.traj_link(traj, tx, params, STEP, capacity=10, bodies=both)
    assert (length == COUNT).all()
    same_bits(got, full[rows, :10], "capacity 10")
    # a transmitter without a stored state
    empty = head(tx, 1)
    empty.len[:] = 0
    got, length, epoch0 = ctx.traj_link(traj, empty, params, STEP, capacity=6, bodies=both)
    assert (length == 0).all() and np.isnan(got).all() and (epoch0 == 0).all()
    # epoch0_ns is optional in the ABI: the same values and lengths without it
    lib = _abi.load_library()
    n, cap = 70, 12
    q = link_query(world, params, both)
    cin, cref = traj.as_c(), tx.as_c()
    vals, ln = np.zeros((3, cap, n)), np.zeros(n, dtype=np.int32)
    assert lib.nyx_hip_traj_link(ctx._h, C.byref(cin), n, C.byref(cref), 1, C.byref(q), cap, vals.ctypes.data_as(_abi.c_double_p),
                                 ln.ctypes.data_as(_abi.c_int32_p), None) == 0, _abi.last_error()
    assert (ln == COUNT).all()
    same_bits(vals, full[rows, :cap], "without epoch0")


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_4_seams_and_shapes(world, leo70, n):
    ctx = world["ctx"]
    lib = _abi.load_library()
    traj, tx, full = head(leo70["traj"], n), leo70["tx"], leo70["got"]
    params = [L.Range, L.RangeRate, L.Visible, L.ObstructingBody, L.Clearance, L.LosX, (L.BodyClearance, 1), (L.BodyObstructs, 0)]
    rows = [row(p) for p in params]
    guard = 1000
    for cap in (TILE - 1, TILE, TILE + 1, COUNT):
        size = 8 * cap * n
        buf = np.full(size + guard, 12345.0)
        length = np.full(n + 8, -7, dtype=np.int32)
        epoch0 = np.full(n + 8, -7, dtype=np.int64)
        q = link_query(world, params, world["both"])
        cin, cref = traj.as_c(), tx.as_c()
        rc = lib.nyx_hip_traj_link(ctx._h, C.byref(cin), n, C.byref(cref), 1, C.byref(q), cap, buf.ctypes.data_as(_abi.c_double_p),
                                   length.ctypes.data_as(_abi.c_int32_p), epoch0.ctypes.data_as(_abi.c_int64_p))
        assert rc == 0, _abi.last_error()
        assert (length[:n] == COUNT).all() and (length[n:] == -7).all()          # produced, not stored
        assert (epoch0[:n] == EPOCH0_NS).all() and (epoch0[n:] == -7).all()
        vals = buf[:size].reshape(8, cap, n)
        same_bits(vals, full[rows, :cap, :n], f"n {n} capacity {cap}")            # every stored slot is the slot of test 1, bit for bit
        assert (buf[size:] == 12345.0).all()                                      # nothing beyond n_params * capacity * n
    # one parameter alone, and a window that starts at sample k: the same bits
    one, _, _ = ctx.traj_link(traj, tx, [L.Clearance], STEP, capacity=COUNT, bodies=world["both"])
    same_bits(one[0], full[row(L.Clearance), :, :n], f"n {n} alone")
    for k in (1, TILE, TILE + 1):
        part, length, epoch0 = ctx.traj_link(traj, tx, params, STEP, EPOCH0_NS + k * STEP, EPOCH0_NS + DUR, bodies=world["both"])
        assert (length == COUNT - k).all() and (epoch0 == EPOCH0_NS + k * STEP).all()
        same_bits(part, full[rows, k:, :n], f"n {n} from sample {k}")


def test_5_a_body_whose_chain_ends_inside_the_span(world):
    """Stored epochs that straddle the end of the Moon's chain: the series ends at the first sample past it, `len` names it, NaN
    follows - as the eclipse report does; the neighbour in the same wave, a day earlier, is unaffected; against the centre alone (no
    chain) nothing ends."""
    ctx = world["ctx"]
    al = world["almanac"]
    chain = eclipse.body_chain(nx.MOON, al, world["central"])
    end_s = min(float(al.segments[s].init_et_s) + float(al.segments[s].interval_s) * al.segments[s].records.shape[0] for s, _ in chain)
    end_ns = int(end_s) * S                                # a whole second at or before the end
    k_n = 24
    t, tx = _abi.TrajBatch(2, k_n), _abi.TrajBatch(2, k_n)
    t.len[:] = tx.len[:] = k_n
    t.epoch_ns[:, 0] = end_ns - 10 * STEP + STEP * np.arange(k_n)
    t.epoch_ns[:, 1] = t.epoch_ns[:, 0] - 86400 * S
    tx.epoch_ns[:] = t.epoch_ns
    r0, v0 = leo_nominal()[:3], leo_nominal()[3:]
    for i in range(2):
        tau = (t.epoch_ns[:, i] - t.epoch_ns[0, i]) / S
        t.state[:3, :, i] = r0[:, None] + v0[:, None] * tau[None, :]            # straight lines: any window interpolates them
        t.state[3:, :, i] = v0[:, None]
        tx.state[:3, :, i] = 1.5 * r0[:, None] - v0[:, None] * tau[None, :]
        tx.state[3:, :, i] = -v0[:, None]
    params = [L.Range, L.Visible, (L.BodyClearance, 1)]
    vals, length, epoch0 = ctx.traj_link(t, tx, params, STEP, capacity=k_n + 3, bodies=world["both"])
    ev, evt = ctx.traj_every(t, STEP, k_n), ctx.traj_every(tx, STEP, k_n)
    assert (ev.len == k_n).all() and (evt.len == k_n).all()                     # every sample CAN be interpolated
    want = host_values(world, params, ev.state.transpose(1, 2, 0), evt.state.transpose(1, 2, 0), ev.epoch_ns, world["both"])
    bad = np.nonzero(np.isnan(want[1, :, 0]))[0]
    assert len(bad) and 8 <= bad[0] <= 12 and not np.isnan(want[:, :, 1]).any() and np.isfinite(want[0]).all()
    assert list(length) == [int(bad[0]), k_n] and list(epoch0) == [int(t.epoch_ns[0, 0]), int(t.epoch_ns[0, 1])]
    assert np.isnan(vals[:, bad[0]:, 0]).all() and np.isnan(vals[:, k_n:, 1]).all()      # later samples included, the Range too
    same_bits(vals[:, :bad[0], 0], want[:, :bad[0], 0], "before the end")
    same_bits(vals[:, :k_n, 1], want[:, :, 1], "neighbour")
    own, l2, _ = ctx.traj_link(t, tx, [L.Range, L.Visible], STEP)               # the default: the centre, no chain
    assert list(l2) == [k_n, k_n] and np.isfinite(own).all()
    same_bits(own[0], want[0], "the centre alone")


def test_6_no_body(world, leo70):
    ctx = world["ctx"]
    params = [L.Visible, L.ObstructingBody, L.Clearance, L.Range, L.RelativeSpeed]
    got, length, _ = ctx.traj_link(leo70["traj"], leo70["tx"], params, STEP, capacity=COUNT + 2, bodies=[])
    assert (length == COUNT).all() and np.isnan(got[:, COUNT:]).all()
    assert (got[0, :COUNT] == 1.0).all() and (got[1, :COUNT] == -1.0).all() and (got[2, :COUNT] == np.inf).all()
    same_bits(got[3:, :COUNT], leo70["got"][[row(L.Range), row(L.RelativeSpeed)]], "no body")
    # and the default - the centre alone - is the Earth's own rows
    got, length, _ = ctx.traj_link(leo70["traj"], leo70["tx"], [L.Visible, L.Clearance, L.ObstructingBody], STEP, capacity=COUNT)
    same_bits(got, leo70["got"][[row(L.Visible), row((L.BodyClearance, 0)), row(L.ObstructingBody)]], "the centre alone")
    lib = _abi.load_library()
    q = link_query(world, [(L.BodyClearance, 0)], [world["central"]])
    q.n_bodies = 0
    cin, cref = leo70["traj"].as_c(), leo70["tx"].as_c()
    vals, ln = np.zeros(70), np.zeros(70, dtype=np.int32)
    assert lib.nyx_hip_traj_link(ctx._h, C.byref(cin), 70, C.byref(cref), 1, C.byref(q), 1, vals.ctypes.data_as(_abi.c_double_p),
                                 ln.ctypes.data_as(_abi.c_int32_p), None) == _abi.RC_BAD_ARG
    assert "names no body" in _abi.last_error() and (vals == 0).all()


def test_7_device_pointers_on_a_stream_behind_the_propagation(world, leo70):
    """propagate_with_traj_device -> traj_link_device on one HIP stream, every buffer a device tensor, no host round trip in between:
    equal to the host entry on the host flavour's trajectories, nothing written beyond n_params * capacity * n doubles."""
    import torch
    ctx = world["ctx"]
    lib = _abi.load_library()
    dev = torch.device("cuda", 0)
    n, cap, guard = 70, 40, 512
    params = [L.Range, L.Visible, (L.BodyClearance, 1)]
    start, stop = EPOCH0_NS + 500 * S, EPOCH0_NS + 5000 * S
    host, host_len, host_epoch0 = ctx.traj_link(leo70["traj"], leo70["tx"], params, STEP, start, stop, capacity=cap, bodies=world["both"])
    b = dispersed_leo_batch(n, seed=11)
    keep = []

    def dev_states(batch):
        t = {"epoch_ns": torch.from_numpy(batch.epoch_ns).to(dev), "step_ns": torch.zeros(batch.n, dtype=torch.int64, device=dev)}
        for f in _abi.F64_FIELDS:
            t[f] = torch.from_numpy(getattr(batch, f)).to(dev)
        s = _abi.States()
        s.n = batch.n
        s.epoch_ns = C.cast(t["epoch_ns"].data_ptr(), _abi.c_int64_p)
        s.step_ns = C.cast(t["step_ns"].data_ptr(), _abi.c_int64_p)
        for f in _abi.F64_FIELDS:
            setattr(s, f, C.cast(t[f].data_ptr(), _abi.c_double_p))
        keep.append(t)
        return s

    def dev_traj(capacity, cols, source=None):
        t = {"epoch": torch.zeros((capacity, cols), dtype=torch.int64, device=dev), "state": torch.zeros((6, capacity, cols), dtype=torch.float64, device=dev),
             "len": torch.zeros(cols, dtype=torch.int32, device=dev)}
        if source is not None:
            t = {"epoch": torch.from_numpy(source.epoch_ns).to(dev), "state": torch.from_numpy(source.state).to(dev), "len": torch.from_numpy(source.len).to(dev)}
        s = _abi.Traj()
        s.capacity = capacity
        s.epoch_ns = C.cast(t["epoch"].data_ptr(), _abi.c_int64_p)
        for k, f in enumerate(["x_km", "y_km", "z_km", "vx_km_s", "vy_km_s", "vz_km_s"]):
            setattr(s, f, C.cast(t["state"][k].data_ptr(), _abi.c_double_p))
        s.len = C.cast(t["len"].data_ptr(), _abi.c_int32_p)
        keep.append(t)
        return s

    sin, sout = dev_states(b), dev_states(b)
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    sst = _abi.StepStats()
    sst.status = C.cast(status.data_ptr(), _abi.c_int32_p)
    straj = dev_traj(256, n)
    stx = dev_traj(leo70["tx"].capacity, 1, leo70["tx"])
    size = 3 * cap * n
    values = torch.full((size + guard,), 12345.0, dtype=torch.float64, device=dev)
    length = torch.full((n + 8,), -7, dtype=torch.int32, device=dev)
    epoch0 = torch.full((n + 8,), -7, dtype=torch.int64, device=dev)
    q = link_query(world, params, world["both"], start=start, stop=stop)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        h = C.c_void_p(stream.cuda_stream)
        assert lib.nyx_hip_propagate_batch_with_traj_device(ctx._h, C.byref(sin), DUR, C.byref(sout), C.byref(sst), C.byref(straj), h) == 0
        rc = lib.nyx_hip_traj_link_device(ctx._h, C.byref(straj), n, C.byref(stx), 1, C.byref(q), cap, C.c_void_p(values.data_ptr()),
                                          C.c_void_p(length.data_ptr()), C.c_void_p(epoch0.data_ptr()), h)
    assert rc == 0, _abi.last_error()
    stream.synchronize()
    assert int((status != 0).sum()) == 0
    got, got_len, got_epoch0 = values.cpu().numpy(), length.cpu().numpy(), epoch0.cpu().numpy()
    np.testing.assert_array_equal(got_len[:n], host_len)
    np.testing.assert_array_equal(got_epoch0[:n], host_epoch0)
    assert (got_len[n:] == -7).all() and (got_epoch0[n:] == -7).all() and (host_len == 76).all()      # (5000 - 500) / 60 + 1 produced, 40 stored
    same_bits(got[:size].reshape(3, cap, n), host, "device entry")
    assert (got[size:] == 12345.0).all() and np.isfinite(host).all()           # guard words: nothing beyond the buffer


def test_8_results_link_views_on_a_real_monte_carlo(world, leo70):
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
    assert isinstance(res.runs[fail].result, nx.PropagationError) and len(res.ok_runs()) == runs - 1
    params = [L.Range, L.RangeRate, L.Visible, L.Clearance, (L.BodyClearance, world["moon"])]
    tx = leo70["tx"]
    series = res.link_views(tx, STEP, params, world["both"])
    ctx = res._traj_ctx
    assert hasattr(ctx, "traj_link")

    class Compose:   # the evaluator of the definition: traj_every / traj_at only, and what the runs were compiled from
        traj_at = staticmethod(ctx.traj_at)
        traj_every = staticmethod(ctx.traj_every)
        compiled = ctx.compiled

    want = dataclasses.replace(res, _traj_ctx=Compose).link_views(tx, STEP, params, world["both"])
    assert isinstance(series, nx.LinkSeries) and series.values.shape == want.values.shape == (5, COUNT, runs)
    for f in ("len", "epoch0_ns", "ok"):
        np.testing.assert_array_equal(getattr(series, f), getattr(want, f))
    assert series.len[fail] == 0 and np.isnan(series.values[:, :, fail]).all() and list(np.delete(series.len, fail)) == [COUNT] * (runs - 1)
    okc = np.nonzero(series.ok)[0]
    same_bits(series.values[:, :, okc], want.values[:, :, okc], "fused against composed")
    frac = series.visible_fraction()
    np.testing.assert_array_equal(frac, series.of(L.Visible)[:, okc].mean(axis=1))
    assert 0.05 <= frac.mean() <= 0.5 and frac.min() == 0.0 and frac.max() == 1.0
    best, when = series.closest_range()
    np.testing.assert_array_equal(best[okc], series.of(L.Range)[:, okc].min(axis=0))
    assert np.isnan(best[fail]) and when[fail] == 0 and ((when[okc] - EPOCH0_NS) % STEP == 0).all()
    # one trajectory through Traj.link_view
    run = res.runs[0].result.traj
    ep, one = run.link_view(nx.Traj(ctx, tx, 0), STEP, params, bodies=world["both"])
    assert list(ep) == [EPOCH0_NS + k * STEP for k in range(COUNT)] and one.shape == (5, COUNT)
    same_bits(one, series.values[:, :, 0], "Traj.link_view")


def test_9_what_the_query_asks_of_the_context_is_refused_through_the_library(world, leo70):
    """A segment index beyond the context's segments: NYX_HIP_RC_BAD_ARG.  A context with an integration-frame swap:
    NYX_HIP_RC_UNSUPPORTED.  Neither launches anything: the outputs are untouched."""
    lib = _abi.load_library()
    ctx, traj, tx = world["ctx"], head(leo70["traj"], 2), leo70["tx"]
    cin, cref = traj.as_c(), tx.as_c()
    values, length = np.zeros(4 * 2), np.zeros(2, dtype=np.int32)
    vp, lp = values.ctypes.data_as(_abi.c_double_p), length.ctypes.data_as(_abi.c_int32_p)
    q = link_query(world, [L.Visible], world["both"])
    q.bodies[1].chain_segment[1] = world["compiled"].cfg.n_segments
    assert lib.nyx_hip_traj_link(ctx._h, C.byref(cin), 2, C.byref(cref), 1, C.byref(q), 4, vp, lp, None) == _abi.RC_BAD_ARG
    assert "bodies[1].chain_segment[1]" in _abi.last_error() and "not a segment of the context" in _abi.last_error()
    swapped = nx.GpuContext(world["prop"].compile(world["almanac"], world["central"], state_frame=world["moon"]))
    try:
        q = link_query(world, [L.Visible], world["both"])
        for fn, extra in ((lib.nyx_hip_traj_link, ()), (lib.nyx_hip_traj_link_device, (None,))):
            assert fn(swapped._h, C.byref(cin), 2, C.byref(cref), 1, C.byref(q), 4, vp, lp, None, *extra) == _abi.RC_UNSUPPORTED
            assert "integration-frame swap" in _abi.last_error()
        with pytest.raises(RuntimeError, match="integration-frame swap"):
            swapped.traj_link(traj, tx, [L.Visible], STEP)
    finally:
        swapped.close()
    assert (values == 0).all() and (length == 0).all()
