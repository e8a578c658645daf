"""The host path of the run entries (host_run in abi.cpp on nyx_amd/csrc/run_host.h) on the device, at the smallest shapes at which
its layout code can go wrong: nyx_hip_predict_until's one working block with every subset of outputs a caller may ask for (a part
that is absent must not move, alias or lose another), nyx_hip_propagate_until_event's event block with and without `crossings`,
the host flavour of nyx_hip_ensemble_moments against the device flavour, and one refusal per entry through the real library (the
header's checks reach the caller).  Everything here is a refusal before any launch or a valid run."""
import ctypes as C

import numpy as np
import pytest

import nyx_amd as nx
import oracle_lib
import predict_cases as pc
from nyx_amd import _abi, od
from scenarios import dispersed_leo_batch, leo_full_setup
from test_oracle_events import period_ns, setup

pytestmark = pytest.mark.gpu
PER_SEGMENT = 0x20000000
HIST = (("epoch_ns", np.int64, 1), ("state", np.float64, 9), ("stm", np.float64, 81), ("covar", np.float64, 81), ("state_dev", np.float64, 9))
CAPACITY = 8   # (shapes_case performs 4 to 6 updates: the last slots of every run stay unwritten)


def predict(ctx, case, arrays=(), capacity=CAPACITY, hist=True, state_dev=True):
    """nyx_hip_predict_until through _abi with exactly the outputs asked for; everything the call wrote, by name.  The arrays start
    as ones: a slot the entry leaves alone shows."""
    batch, n = case["batch"], case["batch"].n
    cfg = od.build_predict(case["max_step"], case["end"], case["noise"], True)
    covar = od._col_major(np.asarray(case["p0"], dtype=np.float64).reshape(n, 9, 9))
    dev = np.ascontiguousarray(case["dev0"], dtype=np.float64).reshape(n, 9).copy()
    est = _abi.Estimates(covar.ctypes.data_as(_abi.c_double_p), dev.ctypes.data_as(_abi.c_double_p) if state_dev else None)
    out, stats = batch.copy(), _abi.StatsBatch(n)
    got = {"n_updates": np.full(n, -1, dtype=np.int32)}
    h = _abi.PredictHistory()
    h.capacity = capacity
    h.n_updates = got["n_updates"].ctypes.data_as(_abi.c_int32_p)
    for name, dtype, width in HIST:
        if name in arrays:
            got["h." + name] = np.ones((max(capacity, 1), n, width), dtype=dtype)
            setattr(h, name, got["h." + name].ctypes.data_as(C.POINTER(C.c_int64 if dtype is np.int64 else C.c_double)))
    cin, cout, cst = batch.as_c(), out.as_c(), stats.as_c()
    rc = ctx._lib.nyx_hip_predict_until(ctx._h, C.byref(cin), C.byref(cfg), C.byref(est), C.byref(cout), C.byref(cst), C.byref(h) if hist else None)
    assert rc == 0, _abi.last_error()
    got.update(covar=covar, rv=out.rv(), epoch=out.epoch_ns, stm_out=out.stm, status=stats.status, n_accepted=stats.n_accepted,
               n_rejected=stats.n_rejected, n_evals=stats.n_evals)
    if state_dev:
        got["dev"] = dev
    return got


@pytest.fixture(scope="module")
def loops():
    prop, almanac, central = leo_full_setup(degree=0)
    compiled = prop.compile(almanac, central, stm=True)
    ctxs = {"fused": nx.GpuContext(compiled), "per_segment": nx.GpuContext(compiled, tuning=nx.Tuning(debug_flags=PER_SEGMENT))}
    yield ctxs
    for c in ctxs.values():
        c.close()


@pytest.mark.parametrize("n", [17, 1])
@pytest.mark.parametrize("loop", ["fused", "per_segment"])
def test_predict_returns_the_same_whatever_subset_of_outputs_is_asked_for(loops, loop, n):
    """shapes_case: degree 0, n = 17 one trajectory more than a workgroup of the quad layout, and n = 1.  All five history arrays
    once; then each alone, none, capacity 0, no history at all, no deviations: every array a variant returns is bit for bit the
    all-arrays run's, n_updates / final covariance / states / counters are equal, the unwritten slots are zero."""
    ctx, case = loops[loop], pc.shapes_case(n)
    names = [name for name, _, _ in HIST]
    full = predict(ctx, case, names)
    assert (full["status"] == 0).all() and full["n_updates"].max() == 6 and full["n_updates"].min() >= 4
    written = np.arange(CAPACITY)[:, None] < full["n_updates"][None, :]
    assert not written.all()
    for name in names:
        assert not full["h." + name][~written].any(), f"{name}: unwritten history slots are not zero"
        assert full["h." + name][written].any(), name
    always = ("covar", "rv", "epoch", "stm_out", "status", "n_accepted", "n_rejected", "n_evals")
    variants = [dict(arrays=(name,)) for name in names] + [dict(arrays=()), dict(arrays=names, capacity=0), dict(arrays=(), hist=False),
                                                           dict(arrays=names, state_dev=False), dict(arrays=(), hist=False, state_dev=False)]
    for v in variants:
        got = predict(ctx, case, **v)
        what = f"{loop} n={n} {v}"
        for k in always:   # (none of these depends on the deviations the filter starts from: zeros when the caller gives none)
            np.testing.assert_array_equal(got[k], full[k], err_msg=f"{what}: {k}")
        if v.get("hist", True):
            np.testing.assert_array_equal(got["n_updates"], full["n_updates"], err_msg=what)
        else:
            assert (got["n_updates"] == -1).all(), what   # (not the entry's to write)
        if v.get("state_dev", True):
            np.testing.assert_array_equal(got["dev"], full["dev"], err_msg=what)
        for name in v["arrays"]:
            if v.get("capacity", CAPACITY) == 0:
                assert (got["h." + name] == 1).all(), f"{what}: {name} written with capacity 0"
            elif name == "state_dev" and not v.get("state_dev", True):
                assert not got["h." + name][~written].any(), f"{what}: {name}"
            else:
                np.testing.assert_array_equal(got["h." + name], full["h." + name], err_msg=f"{what}: {name}")


@pytest.mark.parametrize("n", [1, 3])
def test_until_event_with_and_without_crossings(n):
    """The two-body setup of test_oracle_events, trigger 2, capacity 64 (fewer states than the runs publish: the search then reports
    that it lacks the bracket, for device and oracle alike): the same outputs whether `crossings` is given or NULL; crossings,
    traj.len, status and the stored states equal the oracle's."""
    compiled, batch = setup(n=n)
    ctx = nx.GpuContext(compiled)
    event, cap, dur = nx.Event.apoapsis(), 64, 5 * period_ns(batch.rv()[0])

    def run(with_crossings):
        out, stats, traj, cr = batch.copy(), _abi.StatsBatch(n), _abi.TrajBatch(n, cap), np.full(n, -1, dtype=np.int32)
        cin, cout, cst, ctr, cev = batch.as_c(), out.as_c(), stats.as_c(), traj.as_c(), event.as_c(2)
        rc = ctx._lib.nyx_hip_propagate_until_event(ctx._h, C.byref(cin), dur, C.byref(cev), C.byref(cout), C.byref(cst), C.byref(ctr),
                                                    cr.ctypes.data_as(_abi.c_int32_p) if with_crossings else None)
        assert rc == 0, _abi.last_error()
        return out, stats, traj, cr

    out, st, traj, cr = run(True)
    out2, st2, traj2, cr2 = run(False)
    assert (cr2 == -1).all()
    np.testing.assert_array_equal(out2.rv(), out.rv())
    np.testing.assert_array_equal(out2.epoch_ns, out.epoch_ns)
    np.testing.assert_array_equal(traj2.len, traj.len)
    np.testing.assert_array_equal(traj2.epoch_ns, traj.epoch_ns)
    np.testing.assert_array_equal(traj2.state, traj.state)
    for f in ("status", "n_accepted", "n_rejected", "n_evals"):
        np.testing.assert_array_equal(getattr(st2, f), getattr(st, f), err_msg=f)
    ref, rst, rtraj, rcr = oracle_lib.propagate_until_event(compiled, batch, dur, event, trigger=2, capacity=cap)
    np.testing.assert_array_equal(st.status, rst.status)
    np.testing.assert_array_equal(cr, rcr)
    np.testing.assert_array_equal(traj.len, rtraj.len)            # two-body: bit-identical step sequences
    np.testing.assert_array_equal(st.n_accepted, rst.n_accepted)
    assert (cr == 2).all()
    for i in range(n):
        m = min(int(traj.len[i]), cap)                            # (the states beyond the capacity are counted, not stored)
        np.testing.assert_array_equal(traj.epoch_ns[:m, i], rtraj.epoch_ns[:m, i])
        np.testing.assert_array_equal(traj.state[:, :m, i], rtraj.state[:, :m, i])
    assert (st.status == _abi.ERR_EVENT_SEARCH).all()              # (64 states do not hold the bracket of the second apoapsis)
    ctx.close()


@pytest.mark.parametrize("n", [1, 65])
def test_moments_host_flavour_equals_the_device_flavour(n):
    """Bit for bit, with `status` given and NULL, with the cr / cd / mass rows given and NULL (a fixed grid and summation order)."""
    import torch
    compiled, _ = setup()
    ctx = nx.GpuContext(compiled)
    lib, dev = ctx._lib, torch.device("cuda", 0)
    b = dispersed_leo_batch(n, seed=5)
    b.cr[:] = 1.2 + 0.01 * np.arange(n); b.cd[:] = 2.2 - 0.01 * np.arange(n); b.prop_mass_kg[:] = 100.0 + np.arange(n)
    status = (np.arange(n) % 3 == 1).astype(np.int32) * 7
    x0 = np.array([b.rv()[0, k] for k in range(6)] + [1.2, 2.2, 100.0])
    for with_status in (True, False):
        for with_rows in (True, False):
            cin = b.as_c()
            tensors = {f: torch.from_numpy(getattr(b, f)).to(dev) for f in _abi.F64_FIELDS[:9]}
            din = _abi.States()
            din.n = n
            for k, f in enumerate(_abi.F64_FIELDS[:9]):
                if k >= 6 and not with_rows:
                    setattr(cin, f, None)
                else:
                    setattr(din, f, C.cast(tensors[f].data_ptr(), _abi.c_double_p))
            host = np.zeros(55)
            rc = lib.nyx_hip_ensemble_moments(ctx._h, C.byref(cin), status.ctypes.data_as(_abi.c_int32_p) if with_status else None,
                                              x0.ctypes.data_as(_abi.c_double_p), host.ctypes.data_as(_abi.c_double_p))
            assert rc == 0, _abi.last_error()
            dstatus, dout = torch.from_numpy(status).to(dev), torch.zeros(55, dtype=torch.float64, device=dev)
            rc = lib.nyx_hip_ensemble_moments_device(ctx._h, C.byref(din), C.c_void_p(dstatus.data_ptr()) if with_status else None,
                                                     x0.ctypes.data_as(_abi.c_double_p), C.c_void_p(dout.data_ptr()), None)
            assert rc == 0, _abi.last_error()
            torch.cuda.synchronize()
            np.testing.assert_array_equal(host, dout.cpu().numpy(), err_msg=f"n={n} status={with_status} rows={with_rows}")
            assert host[0] == ((status == 0).sum() if with_status else n)
    ctx.close()


def test_each_entrys_checks_reach_the_caller():
    """One refusal per entry through the real library: return code and a fragment of the message."""
    compiled, batch = setup(n=3)
    ctx = nx.GpuContext(compiled)
    lib, n = ctx._lib, batch.n
    out, stats = batch.copy(), _abi.StatsBatch(n)
    cin, cout, cst = batch.as_c(), out.as_c(), stats.as_c()
    traj = _abi.TrajBatch(n, 4)
    ctr = traj.as_c()
    # until_event: trigger 0
    cev = nx.Event.apoapsis().as_c(0)
    assert lib.nyx_hip_propagate_until_event(ctx._h, C.byref(cin), 10**12, C.byref(cev), C.byref(cout), C.byref(cst), C.byref(ctr), None) == 1
    assert "trigger >= 1" in _abi.last_error()
    # predict: n_process_noise -1 (on an STM context: the flag is checked first)
    prop, almanac, central = leo_full_setup(degree=0)
    stm_ctx = nx.GpuContext(prop.compile(almanac, central, stm=True))
    cfg = od.build_predict(60 * nx.NS_PER_S, int(batch.epoch_ns[0]) + 60 * nx.NS_PER_S)
    cfg.n_process_noise = -1
    covar = np.zeros((n, 81))
    est = _abi.Estimates(covar.ctypes.data_as(_abi.c_double_p), None)
    assert lib.nyx_hip_predict_until(stm_ctx._h, C.byref(cin), C.byref(cfg), C.byref(est), C.byref(cout), C.byref(cst), None) == 1
    assert "n_process_noise out of range" in _abi.last_error()
    stm_ctx.close()
    # sharded: out->n != in->n
    small = batch.slice(0, 2)
    csmall = small.as_c()
    arr = (C.c_void_p * 1)(ctx._h)
    assert lib.nyx_hip_propagate_batch_sharded(arr, 1, C.byref(cin), 10**9, C.byref(csmall), C.byref(cst), None) == 1
    assert "out->n != in->n" in _abi.last_error()
    # with_traj: capacity 0
    ctr.capacity = 0
    assert lib.nyx_hip_propagate_batch_with_traj(ctx._h, C.byref(cin), 10**9, C.byref(cout), C.byref(cst), C.byref(ctr)) == 1
    assert "capacity >= 1" in _abi.last_error()
    ctx.close()
