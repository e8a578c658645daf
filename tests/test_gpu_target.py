"""The fused targeter loop on the MI355X (target_kernel.hip, include/nyx_hip_target.h).

THE REFERENCE of every comparison is the host definition (`nyx_amd.targeter.target_definition`) DRIVEN BY THE SAME DEVICE PROPAGATOR:
`propagate_fn = ctx.propagate_until_epoch` on a context with `tuning.deterministic = 1`, whose bits per trajectory do not depend on
the batch.  The fused loop propagates the same start states with the same kernel, so its final states are the reference's bit for
bit, and what follows is csrc/target_dev.h against nyx_amd/targeter.py: the objectives used here (Eccentricity, SemiMajorAxis,
BdotT, BdotR, Rmag, X) are among the twenty parameters tests/test_gpu_frame.py holds to a bound of ZERO (+ - * / sqrt and fabs only,
one order on both sides, -ffp-contract=off), the Newton step is the same kind of arithmetic: status, iterations, correction, errors,
corrected and achieved states are compared for EQUAL BITS.  Small on purpose: at most 257 runs, half an orbit."""
import ctypes as C

import numpy as np
import pytest

import nyx_amd as nx
import target_cases as tc
from nyx_amd import _abi, frames
from nyx_amd.frames import FrameParameter as FP
from nyx_amd.targeter import Objective, TargetStatus, Targeter, Variable, Vary, target_definition
from scenarios import dispersed_leo_batch, leo_full_setup

pytestmark = pytest.mark.gpu

S = nx.NS_PER_S
SIZES = (1, 65, 130, 257)   # one lane; a partial second wave; three waves; a second workgroup


def bits(a):
    """The bit patterns of an array of doubles, every NaN as ONE pattern (a NaN's sign and payload are not part of any definition)."""
    a = np.array(a, dtype=np.float64)
    a[np.isnan(a)] = np.nan
    return np.ascontiguousarray(a).view(np.uint64)


def assert_same_solution(got, want, rows=None, label=""):
    """Every output of two TargeterSolutions, bit for bit (`rows`: the runs of `want` that `got` holds)."""
    rows = np.arange(got.n) if rows is None else np.asarray(rows)
    np.testing.assert_array_equal(got.status, want.status[rows], err_msg=f"status{label}")
    np.testing.assert_array_equal(got.iterations, want.iterations[rows], err_msg=f"iterations{label}")
    np.testing.assert_array_equal(bits(got.correction), bits(want.correction[:, rows]), err_msg=f"correction{label}")
    np.testing.assert_array_equal(bits(got.achieved_errors), bits(want.achieved_errors[:, rows]), err_msg=f"achieved_errors{label}")
    np.testing.assert_array_equal(bits(got.corrected.rv()), bits(want.corrected.rv()[rows]), err_msg=f"corrected{label}")
    np.testing.assert_array_equal(bits(got.achieved.rv()), bits(want.achieved.rv()[rows]), err_msg=f"achieved{label}")
    np.testing.assert_array_equal(got.corrected.epoch_ns, want.corrected.epoch_ns[rows])
    np.testing.assert_array_equal(got.achieved.epoch_ns, want.achieved.epoch_ns[rows])
    for f in _abi.F64_FIELDS[6:]:
        np.testing.assert_array_equal(getattr(got.corrected, f), getattr(want.corrected, f)[rows], err_msg=f)
        np.testing.assert_array_equal(getattr(got.achieved, f), getattr(want.achieved, f)[rows], err_msg=f)


def fused_device(ctx, batch, variables, objectives, t0, t1, **kw):
    """nyx_hip_target_batch_device on torch tensors and a stream of its own; guard words behind every output."""
    import torch
    lib, dev = _abi.load_library(), torch.device("cuda", 0)
    q = ctx.target_query(variables, objectives, t0, t1, **kw)
    n, V, O, guard = batch.n, len(variables), len(objectives), 16
    rows = torch.from_numpy(np.stack([getattr(batch, f) for f in _abi.F64_FIELDS])).to(dev)
    epoch = torch.from_numpy(batch.epoch_ns.copy()).to(dev)

    def states(ep, rw):
        s = _abi.States()
        s.n = n
        s.epoch_ns = C.cast(C.c_void_p(ep.data_ptr()), _abi.c_int64_p)
        for k, f in enumerate(_abi.F64_FIELDS):
            setattr(s, f, C.cast(C.c_void_p(rw[k].data_ptr()), _abi.c_double_p))
        return s
    status = torch.full((n + guard,), -7, dtype=torch.int32, device=dev)
    its = torch.full((n + guard,), -7, dtype=torch.int32, device=dev)
    corr = torch.full((V * n + guard,), 12345.0, dtype=torch.float64, device=dev)
    errs = torch.full((O * n + guard,), 12345.0, dtype=torch.float64, device=dev)
    out_rows = [torch.full((13, n + guard), 12345.0, dtype=torch.float64, device=dev) for _ in range(2)]
    out_epoch = [torch.full((n + guard,), -7, dtype=torch.int64, device=dev) for _ in range(2)]
    res = _abi.TargetResult()
    res.status, res.iterations = C.cast(C.c_void_p(status.data_ptr()), _abi.c_int32_p), C.cast(C.c_void_p(its.data_ptr()), _abi.c_int32_p)
    res.correction, res.achieved_errors = C.cast(C.c_void_p(corr.data_ptr()), _abi.c_double_p), C.cast(C.c_void_p(errs.data_ptr()), _abi.c_double_p)
    res.corrected, res.achieved = states(out_epoch[0], out_rows[0]), states(out_epoch[1], out_rows[1])
    cin = states(epoch, rows)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        rc = lib.nyx_hip_target_batch_device(ctx._h, C.byref(cin), C.byref(q), C.byref(res), C.c_void_p(stream.cuda_stream))
    assert rc == 0, _abi.last_error()
    stream.synchronize()
    for t, fill in ((status, -7), (its, -7), (corr, 12345.0), (errs, 12345.0), (out_epoch[0], -7), (out_epoch[1], -7)):
        assert (t[-guard:] == fill).all()                 # nothing written past the arrays
    assert (out_rows[0][:, n:] == 12345.0).all() and (out_rows[1][:, n:] == 12345.0).all()
    packs = []
    for ep, rw in zip(out_epoch, out_rows):
        b = _abi.StateBatch(n)
        b.epoch_ns[:] = ep[:n].cpu().numpy()
        host = rw[:, :n].cpu().numpy()
        for k, f in enumerate(_abi.F64_FIELDS):
            getattr(b, f)[:] = host[k]
        packs.append(b)
    from nyx_amd.targeter import TargeterSolutions
    return TargeterSolutions(variables, objectives, status[:n].cpu().numpy(), its[:n].cpu().numpy(), corr[:V * n].cpu().numpy().reshape(V, n),
                             errs[:O * n].cpu().numpy().reshape(O, n), packs[0], packs[1], res.iterations_run)


@pytest.fixture(scope="module")
def world():
    ctx = nx.GpuContext(tc.two_body_compiled(), tuning=nx.Tuning(deterministic=1))
    yield dict(ctx=ctx)
    ctx.close()


@pytest.fixture(scope="module")
def ensemble(world):
    """257 states dispersed about the orbit (sigma 1 km, 1 m/s, a fixed seed) and the host-driven loop on them: computed once."""
    c = tc.CASES["sma_ecc"]
    batch = tc.dispersed(257)
    t0, t1 = tc.EPOCH, tc.EPOCH + c["dur_ns"]
    want = target_definition(world["ctx"].propagate_until_epoch, batch, c["variables"], c["objectives"], t0, t1, tc.MU)
    assert (want.status == 0).all()
    print("iterations of the ensemble:", dict(zip(*np.unique(want.iterations, return_counts=True))))
    return c, batch, t0, t1, want


@pytest.mark.parametrize("flavour", ["host", "device"])
@pytest.mark.parametrize("n", SIZES)
def test_8_fused_loop_equals_the_host_driven_loop(world, ensemble, n, flavour):
    c, batch, t0, t1, want = ensemble
    ctx, part = world["ctx"], batch.slice(0, n)
    if flavour == "host":
        got = ctx.target(part, c["variables"], c["objectives"], t0, t1)
    else:
        got = fused_device(ctx, part, c["variables"], c["objectives"], t0, t1)
    assert_same_solution(got, want, np.arange(n), f" n={n} {flavour}")
    assert got.iterations_run == want.iterations[:n].max() + 1
    if n >= 130:
        assert len(set(got.iterations)) >= 2          # runs end at different rounds: the freezing is exercised


def test_9_self_validation_and_the_reference_numbers(world, ensemble):
    c, batch, t0, t1, _ = ensemble
    ctx, part = world["ctx"], batch.slice(0, 65)
    sol = ctx.target(part, c["variables"], c["objectives"], t0, t1)
    assert sol.converged.all()
    tc.check_converged(sol, ctx.propagate_until_epoch, part, c, t0, t1)
    # the reference's two acceptance numbers, through the C-ABI (nyx_amd.Targeter)
    one = Targeter(ctx, c["variables"], c["objectives"]).try_achieve_from(tc.batch_of(tc.RV0), t0, t1)
    dv = float(one.delta_v_norm()[0])
    print(f"sma_ecc: {one.iterations[0]} iterations, |dv| = {dv:.6f} km/s (GMAT {tc.GMAT_SMA_ECC_DV})")
    assert one.status[0] == 0 and (dv < tc.GMAT_SMA_ECC_DV or abs(dv - tc.GMAT_SMA_ECC_DV) < 1e-6)
    b = tc.CASES["bplane"]
    hyp = Targeter.delta_v(ctx, b["objectives"]).try_achieve_from(tc.batch_of(tc.RV_HYP), tc.EPOCH, tc.EPOCH)
    dv = float(hyp.delta_v_norm()[0])
    print(f"bplane: {hyp.iterations[0]} iterations, |dv| = {dv:.6f} km/s (GMAT {tc.GMAT_BPLANE_DV})")
    assert hyp.status[0] == 0 and abs(dv - tc.GMAT_BPLANE_DV) < 1e-3


def test_10_one_ellipse_among_hyperbolas(world):
    """n = 65: 64 dispersed states of the B-plane case and one state of the ellipse among them.  That run is NOT_FINITE at iteration 0,
    the others converge exactly as they do without it."""
    ctx, b = world["ctx"], tc.CASES["bplane"]
    hyp = tc.dispersed(64, seed=9, rv=tc.RV_HYP)
    rv = np.insert(hyp.rv(), 40, tc.RV0, axis=0)
    mixed = tc.batch_of(rv, 65)
    alone = ctx.target(hyp, b["variables"], b["objectives"], tc.EPOCH, tc.EPOCH)
    got = ctx.target(mixed, b["variables"], b["objectives"], tc.EPOCH, tc.EPOCH)
    assert alone.converged.all()
    assert got.status[40] == int(TargetStatus.NOT_FINITE) and got.iterations[40] == 0 and np.isnan(got.achieved_errors[:, 40]).all()
    others = np.delete(np.arange(65), 40)
    for name in ("status", "iterations"):
        np.testing.assert_array_equal(getattr(got, name)[others], getattr(alone, name))
    np.testing.assert_array_equal(bits(got.correction[:, others]), bits(alone.correction))
    np.testing.assert_array_equal(bits(got.achieved_errors[:, others]), bits(alone.achieved_errors))
    np.testing.assert_array_equal(bits(got.corrected.rv()[others]), bits(alone.corrected.rv()))
    want = target_definition(ctx.propagate_until_epoch, mixed, b["variables"], b["objectives"], tc.EPOCH, tc.EPOCH, tc.MU)
    assert_same_solution(got, want)


@pytest.fixture(scope="module")
def moon_world():
    """The small almanac of the GPU suite with the Sun and the Moon as point masses: the objective frame's chain has two segments."""
    prop, almanac, central = leo_full_setup(degree=0, srp=False)
    ctx = nx.GpuContext(prop.compile(almanac, central), tuning=nx.Tuning(deterministic=1))
    yield dict(ctx=ctx, almanac=almanac, central=central, moon=almanac.frame_info(nx.MOON))
    ctx.close()


def test_11_objective_frame_about_the_moon(moon_world):
    """An engineered case (the reference's B-plane targeter test of this shape is #[ignore]d: it holds no number): the aim point is
    what the uncorrected first run achieves about the Moon half an hour later, moved by (+300, -200) km."""
    ctx, almanac, central, moon = (moon_world[k] for k in ("ctx", "almanac", "central", "moon"))
    batch = dispersed_leo_batch(3, seed=4)
    t0, t1 = int(batch.epoch_ns[0]), int(batch.epoch_ns[0]) + 1800 * S
    final, st = ctx.propagate_until_epoch(batch.slice(0, 1), t1)
    assert st.status[0] == 0
    bt, br = (float(frames.frame_value(p, final.rv(), t1, moon, almanac, central)[0]) for p in (FP.BdotT, FP.BdotR))
    objectives = [Objective.within_tolerance(FP.BdotT, bt + 300.0, 1.0), Objective.within_tolerance(FP.BdotR, br - 200.0, 1.0)]
    variables = tc.vel()
    got = ctx.target(batch, variables, objectives, t0, t1, objective_frame=moon)
    want = target_definition(ctx.propagate_until_epoch, batch, variables, objectives, t0, t1, tc.MU, objective_target=moon, almanac=almanac, central=central)
    print("about the Moon:", list(got.status), list(got.iterations), got.delta_v_norm())
    assert want.converged.all()
    assert_same_solution(got, want)
    tc.check_converged(got, ctx.propagate_until_epoch, batch, dict(variables=variables, objectives=objectives), t0, t1, mu=float(moon.mu_km3_s2),
                       about=lambda rv, ep: frames.to_frame(rv, ep, moon, almanac, central))
    # an achievement epoch outside the table: every run EPHEM_RANGE at iteration 0, one round
    late = batch.copy()
    chain = frames.check_target(moon, almanac, central)
    ends = [float(almanac.segments[k].init_et_s) + float(almanac.segments[k].interval_s) * len(almanac.segments[k].records) for k, _ in chain]
    late.epoch_ns[:] = nx.seconds(min(ends) - 600.0)         # ten minutes before the Moon's segments end
    t0 = int(late.epoch_ns[0])
    out = ctx.target(late, variables, objectives, t0, t0 + 1800 * S, objective_frame=moon)
    assert (out.status == int(TargetStatus.EPHEM_RANGE)).all() and (out.iterations == 0).all() and out.iterations_run == 1
    assert np.isnan(out.achieved_errors).all()
    # without an objective frame the same epochs are a propagation failure (the point masses leave the table)
    out = ctx.target(late, variables, tc.SMA_ECC, t0, t0 + 1800 * S)
    assert (out.status == int(TargetStatus.PROP_FAILED)).all() and (out.iterations == 0).all() and out.iterations_run == 1


@pytest.mark.parametrize("name", ["singular", "ineffective", "too_many", "vnc", "delta_r", "sma_only", "one_var_two_objs", "backward", "guess"])
def test_12_cases_on_the_device(world, name):
    """n = 2 of every remaining case against the host-driven loop; `iterations_run` is the largest run's count plus one; a second
    call gives equal bits."""
    ctx, c = world["ctx"], tc.CASES[name]
    rv = np.tile(np.asarray(c["rv"]), (2, 1))
    rv[1, :3] += np.array([0.5, -0.25, 0.125])
    batch = tc.batch_of(rv, 2)
    kw = dict(correction_frame=c.get("frame"), iterations=c.get("iterations", 100))
    t0, t1 = tc.EPOCH, tc.EPOCH + c["dur_ns"]
    got = ctx.target(batch, c["variables"], c["objectives"], t0, t1, **kw)
    want = target_definition(ctx.propagate_until_epoch, batch, c["variables"], c["objectives"], t0, t1, tc.MU, **kw)
    assert got.status[0] == int(c["status"]), TargetStatus(int(got.status[0])).name
    assert_same_solution(got, want, label=f" {name}")
    assert got.iterations_run == got.iterations.max() + 1 == want.iterations_run
    if c["status"] == TargetStatus.OK_CONVERGED:      # item 9's rule: the correction applied independently holds (in the VNC frame too)
        assert got.converged.all()
        tc.check_converged(got, ctx.propagate_until_epoch, batch, c, t0, t1)
    again = ctx.target(batch, c["variables"], c["objectives"], t0, t1, **kw)
    assert_same_solution(again, got, label=f" {name} again")


def test_12_the_context_still_propagates_with_unchanged_results(world):
    """The work block must not disturb the staging blocks: a propagation before and after a targeter call gives equal bits."""
    ctx, c = world["ctx"], tc.CASES["sma_ecc"]
    batch = tc.dispersed(70, seed=3)
    before, st0 = ctx.propagate(batch, 3000 * S)
    ctx.target(batch.slice(0, 33), c["variables"], c["objectives"], tc.EPOCH, tc.EPOCH + c["dur_ns"])
    after, st1 = ctx.propagate(batch, 3000 * S)
    assert (st0.status == 0).all() and (st1.status == 0).all()
    np.testing.assert_array_equal(bits(before.rv()), bits(after.rv()))
    np.testing.assert_array_equal(before.epoch_ns, after.epoch_ns)
