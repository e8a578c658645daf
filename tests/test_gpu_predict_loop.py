"""The one-launch covariance-mapping loop (pk_segment_update.h, the re-arming in role_loop, nyx_hip_predict_until's bookkeeping) at every
workgroup shape, batch edge and exit path: bit for bit against the launch-per-segment loop (debug_flags 0x20000000, nyx_time_update_kernel),
against the oracle at the project's bounds (1e-9 on Phi, P-bar and the deviation, 1e-3 km / 1e-6 km/s on the states) wherever the step
sequence is fixed by construction, and against the time update recomputed in extended precision from the device's own Phi (1e-12, the
bound the oracle itself meets with a factor four to spare: test_predict_cases.py).  Inputs: predict_cases.py."""
import numpy as np
import pytest

import nyx_amd as nx
import oracle_lib
import predict_cases as pc
from nyx_amd import _abi
from scenarios import leo_full_setup

pytestmark = pytest.mark.gpu
PER_SEGMENT = 0x20000000
HISTORY = ("epochs_ns", "nominal", "stm", "covar_history", "deviation_history")
COUNTERS = ("n_accepted", "n_rejected", "n_evals")


class Loops:
    """The default context (one launch) and the launch-per-segment context of one compiled force model."""

    def __init__(self, compiled):
        self.compiled = compiled
        self.fused = nx.GpuContext(compiled)
        self.per_segment = nx.GpuContext(compiled, tuning=nx.Tuning(debug_flags=PER_SEGMENT))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.fused.close()
        self.per_segment.close()

    def both(self, case, what=""):
        """The case through both loops, asserted bit-identical; -> the one-launch result."""
        a, r = device(self.fused, case), device(self.per_segment, case)
        assert_identical(a, r, what)
        return a


def device(ctx, case, noise=None, keep_stm=True):
    kw = pc.kwargs(case, keep_stm)
    if noise is not None:
        kw["process_noise"] = noise
    return nx.predict_until(ctx, case["batch"], case["p0"], case["end"], case["max_step"], **kw)


def oracle(compiled, case, noise=None):
    kw = pc.kwargs(case)
    if noise is not None:
        kw["process_noise"] = noise
    return oracle_lib.predict_until(compiled, case["batch"], case["p0"], case["end"], case["max_step"], **kw)


def kept(res):
    """[slots, n] mask of the history slots a run has filled."""
    cap = res.epochs_ns.shape[0]
    return np.arange(cap)[:, None] < np.minimum(res.n_updates, cap)[None, :]


def assert_identical(a, r, what=""):
    """Every field of two Predicted, bit for bit; the history slots a run has not filled are zero, as the oracle leaves them."""
    np.testing.assert_array_equal(a.n_updates, r.n_updates, err_msg=what)
    np.testing.assert_array_equal(a.stats.status, r.stats.status, err_msg=what)
    np.testing.assert_array_equal(a.states.rv(), r.states.rv(), err_msg=what)
    np.testing.assert_array_equal(a.states.epoch_ns, r.states.epoch_ns, err_msg=what)
    np.testing.assert_array_equal(a.states.stm, r.states.stm, err_msg=what)
    np.testing.assert_array_equal(a.covar, r.covar, err_msg=what)
    np.testing.assert_array_equal(a.state_deviation, r.state_deviation, err_msg=what)
    unfilled = ~kept(a)
    for f in HISTORY:
        if getattr(a, f) is not None or getattr(r, f) is not None:
            np.testing.assert_array_equal(getattr(a, f), getattr(r, f), err_msg=f"{what} {f}")
            assert not getattr(a, f)[unfilled].any(), f"{what} {f}: unfilled history slots are not zero"
    for f in COUNTERS:
        np.testing.assert_array_equal(getattr(a.stats, f), getattr(r.stats, f), err_msg=f"{what} {f}")


def state_errors(got, ref, runs=slice(None)):
    d = got.states.rv()[runs] - ref.states.rv()[runs]
    return np.linalg.norm(d[:, :3], axis=1).max(), np.linalg.norm(d[:, 3:], axis=1).max()


def assert_epochs_equal(got, ref):
    np.testing.assert_array_equal(got.stats.status, ref.stats.status)
    np.testing.assert_array_equal(got.n_updates, ref.n_updates)
    np.testing.assert_array_equal(got.states.epoch_ns, ref.states.epoch_ns)
    m = kept(ref)
    np.testing.assert_array_equal(got.epochs_ns[m], ref.epochs_ns[m])


def oracle_errors(got, ref, runs=None):
    """(Phi, P-bar history, final P-bar, deviation) errors against the oracle over the filled history slots of `runs` (default: all)."""
    m = kept(ref)
    if runs is not None:
        only = np.zeros(m.shape[1], dtype=bool)
        only[runs] = True
        m = m & only[None, :]
        runs = np.flatnonzero(only & (ref.n_updates > 0))
    else:
        runs = np.flatnonzero(ref.n_updates > 0)
    e_dev = max(pc.dev_err(got.deviation_history[m], ref.deviation_history[m]), pc.dev_err(got.state_deviation[runs], ref.state_deviation[runs]))
    return pc.rel_err(got.stm[m], ref.stm[m]), pc.rel_err(got.covar_history[m], ref.covar_history[m]), pc.rel_err(got.covar[runs], ref.covar[runs]), e_dev


def assert_vs_oracle(got, ref, what, runs=None):
    e_phi, e_p, e_last, e_dev = oracle_errors(got, ref, runs)
    dr, dv = state_errors(got, ref, slice(None) if runs is None else runs)
    print(f"{what}: vs the oracle Phi {e_phi:.2e} Pbar {e_p:.2e} last Pbar {e_last:.2e} dev {e_dev:.2e} dr {dr:.2e} km dv {dv:.2e} km/s")
    assert dr < 1e-3 and dv < 1e-6
    assert e_phi < 1e-9 and e_p < 1e-9 and e_last < 1e-9 and e_dev < 1e-9


def assert_vs_reference(got, case, what, noise=None):
    e_p, e_d = pc.reference_errors(got, case["p0"], case["batch"].epoch_ns, case["noise"] if noise is None else noise, case["dev0"])
    print(f"{what}: vs the extended-precision time update of the device's own Phi: Pbar {e_p:.2e} dev {e_d:.2e}")
    assert e_p <= 1e-12 and e_d <= 1e-12


@pytest.mark.parametrize("degree", [0, 4, 21])
def test_workgroup_shapes_and_batch_edges(degree):
    """The three workgroup shapes of the quad kernel - no harmonics (the role workgroup: five or six trajectories' updates per wave),
    degree 4 (eight waves: two per wave, the LDS scratch reused across the trailing wave barrier), degree 21 (sixteen waves: one each) -
    at n = 1, 16, 17 and 33: one trajectory, a full workgroup, a workgroup of one, two and one.  GEO, 60 s segments that are single RK89
    attempts for device and oracle alike, ragged starts (4 to 6 updates, the history keeps 4), decaying RIC noise, deviation tracking."""
    prop, almanac, central = leo_full_setup(degree=degree)
    with Loops(prop.compile(almanac, central, stm=True)) as loops:
        for n in pc.SHAPE_SIZES:
            case, what = pc.shapes_case(n), f"degree {degree} n {n}"
            got = loops.both(case, what)
            ref = oracle(loops.compiled, case)
            assert (got.stats.status == 0).all() and got.n_updates.max() == 6 and got.n_updates.min() >= 4
            assert_epochs_equal(got, ref)
            np.testing.assert_array_equal(got.stats.n_accepted, ref.stats.n_accepted)
            np.testing.assert_array_equal(got.states.stm, np.tile(np.eye(9).ravel(), (n, 1)))
            assert_vs_oracle(got, ref, what)
            assert_vs_reference(got, case, what)
            if degree == 4 and n == 17:
                # no Phi history asked for (hist->stm null) with noise and deviations: the same covariances
                bare = device(loops.fused, case, keep_stm=False)
                assert bare.stm is None
                for f in ("covar_history", "deviation_history", "epochs_ns", "nominal", "covar", "state_deviation", "n_updates"):
                    np.testing.assert_array_equal(getattr(bare, f), getattr(got, f), err_msg=f)


@pytest.mark.parametrize("degree", [8, 0])
def test_adaptive_segments_of_many_attempts(degree):
    """LEO, RK89 with its default options, 600 s segments: about ten accepted steps per segment and rejections among them, the step size
    carried from segment to segment, the counters running over the whole loop - n = 33, ragged starts (5 or 6 updates).  The two device
    loops agree bit for bit.  With the oracle only the states are compared: the reference's STM scheme is first order per step, and one
    ulp on the initial state moves the oracle's own Phi of a 600 s adaptive LEO segment by 2 to 9 % (position: 8e-8 km) even where the
    accepted / rejected counts stay - Phi and P-bar are comparable with the oracle only where the step sequence is fixed by construction.
    The time-update algebra is held to the extended-precision recomputation on the device's own Phi instead."""
    prop, almanac, central = leo_full_setup(degree=degree)
    with Loops(prop.compile(almanac, central, stm=True)) as loops:
        case, what = pc.adaptive_case(), f"adaptive degree {degree}"
        got = loops.both(case, what)
        ref = oracle(loops.compiled, case)
        print(f"{what}: accepted {got.stats.n_accepted.min()}..{got.stats.n_accepted.max()} rejected {got.stats.n_rejected.min()}.."
              f"{got.stats.n_rejected.max()} for {got.n_updates.min()}..{got.n_updates.max()} updates (oracle: rejected "
              f"{ref.stats.n_rejected.min()}..{ref.stats.n_rejected.max()})")
        assert (got.stats.status == 0).all() and got.n_updates.min() == 5 and got.n_updates.max() == 6
        assert (got.stats.n_accepted > 5 * got.n_updates).all()
        assert (got.stats.n_rejected > 0).any()
        assert_epochs_equal(got, ref)
        dr, dv = state_errors(got, ref)
        print(f"{what}: vs the oracle dr {dr:.2e} km dv {dv:.2e} km/s")
        assert dr < 1e-3 and dv < 1e-6
        assert_vs_reference(got, case, what)


@pytest.mark.parametrize("degree", [4, 0])
def test_fixed_step_segments_of_several_steps(degree):
    """RK4 at a fixed 10 s, 30 s segments of three steps ("the final fixed step" of the kernel's re-arming), LEO, n = 33, ragged starts
    (4 or 5 updates): the step sequence is fixed, so every counter equals the oracle's and Phi, P-bar and the deviation meet 1e-9."""
    prop, almanac, central = pc.fixed_step_setup(degree)
    with Loops(prop.compile(almanac, central, stm=True)) as loops:
        case, what = pc.fixed_case(), f"fixed step degree {degree}"
        got = loops.both(case, what)
        ref = oracle(loops.compiled, case)
        assert (got.stats.status == 0).all() and got.n_updates.min() == 4 and got.n_updates.max() == 5
        assert_epochs_equal(got, ref)
        np.testing.assert_array_equal(got.stats.n_accepted, 3 * got.n_updates)
        for f in COUNTERS:
            np.testing.assert_array_equal(getattr(got.stats, f), getattr(ref.stats, f), err_msg=f)
        assert_vs_oracle(got, ref, what)
        assert_vs_reference(got, case, what)


@pytest.mark.parametrize("degree", [0, 4])
def test_a_run_that_fails_in_a_later_segment(degree):
    """Runs that leave the almanac's coverage after zero to three good updates while their workgroup-mates go on or finish (the st != 0
    branch of segment_update, then dur == 0 at every later boundary): n = 20, a full workgroup and a partial one.  The ephemeris error
    is an ordinary per-run status.  The scenario is pinned on the oracle in test_predict_cases.py."""
    prop, almanac, central = pc.fixed_step_setup(degree)
    with Loops(prop.compile(almanac, central, stm=True)) as loops:
        n = 20
        case, what = pc.failure_case(almanac, n), f"failure degree {degree}"
        got = loops.both(case, what)
        ref = oracle(loops.compiled, case)
        print(f"{what}: status {got.stats.status[:8].tolist()} n_updates {got.n_updates[:8].tolist()}")
        assert_epochs_equal(got, ref)
        ok, failed = np.flatnonzero(ref.stats.status == 0), np.flatnonzero(ref.stats.status == _abi.ERR_EPHEM_RANGE)
        assert len(ok) + len(failed) == n and (ref.n_updates[ok] >= 3).any() and (ref.n_updates[failed] == 0).any()
        assert ((ref.n_updates[failed] >= 1) & (ref.n_updates[failed] <= 3)).any()
        assert_vs_oracle(got, ref, what + " finished runs", ok)
        some = failed[ref.n_updates[failed] > 0]
        m = kept(ref)[:, some]
        e_last, e_hist = pc.rel_err(got.covar[some], ref.covar[some]), pc.rel_err(got.covar_history[:, some][m], ref.covar_history[:, some][m])
        e_phi = pc.rel_err(got.stm[:, some][m], ref.stm[:, some][m])
        print(f"{what} failed runs: vs the oracle Phi {e_phi:.2e} Pbar {e_hist:.2e} last Pbar {e_last:.2e}")
        assert e_last < 1e-9 and e_hist < 1e-9 and e_phi < 1e-9
        for i in failed:
            u = got.n_updates[i]
            np.testing.assert_array_equal(got.covar[i], got.covar_history[u - 1, i] if u else case["p0"][i])
            np.testing.assert_array_equal(got.state_deviation[i], got.deviation_history[u - 1, i] if u else case["dev0"][i])
        np.testing.assert_array_equal(got.stats.n_accepted[ok], ref.stats.n_accepted[ok])
        assert_vs_reference(got, case, what)


@pytest.mark.parametrize("kind", ["disable", "late", "init_epoch"])
def test_process_noise_selection(kind):
    """The selections of filtering.rs:64-80 that no other device test reaches (predict_cases.selection_case; n = 17, degree 4, GEO, four
    60 s updates): a last entry passed over for its disable time at every update, an entry that starts after the second update, and an
    explicit ProcessNoise::init_epoch on a decaying entry."""
    prop, almanac, central = leo_full_setup(degree=4)
    with Loops(prop.compile(almanac, central, stm=True)) as loops:
        case = pc.selection_case(kind)
        got = loops.both(case, kind)
        ref = oracle(loops.compiled, case)
        assert (got.stats.status == 0).all() and (got.n_updates == 4).all()
        assert_epochs_equal(got, ref)
        np.testing.assert_array_equal(got.stats.n_accepted, ref.stats.n_accepted)
        assert_vs_oracle(got, ref, kind)
        assert_vs_reference(got, case, kind)
        if case["twin"] is not None:
            twin, u = device(loops.fused, case, noise=case["twin"]), case["twin_updates"]
            np.testing.assert_array_equal(got.covar_history[u], twin.covar_history[u])
            np.testing.assert_array_equal(got.stm, twin.stm)
            if kind == "late":   # and the noise is there from the third update on
                assert (got.covar_history[2, :, 3, 3] > twin.covar_history[2, :, 3, 3]).all()
            else:
                np.testing.assert_array_equal(got.covar, twin.covar)
                assert (got.covar_history[0, :, 3, 3] > device(loops.fused, case, noise=[]).covar_history[0, :, 3, 3]).all()


def test_the_64_lane_layout_through_the_time_update_kernel():
    """stm_quad = 0: sixty-four trajectories per workgroup, the launch-per-segment loop through nyx_time_update_kernel on the other
    workgroup shape - the shapes case at degree 4, n = 17, against the oracle and the extended-precision time update."""
    prop, almanac, central = leo_full_setup(degree=4)
    compiled = prop.compile(almanac, central, stm=True)
    ctx = nx.GpuContext(compiled, tuning=nx.Tuning(stm_quad=0))
    try:
        case, what = pc.shapes_case(17), "64-lane layout"
        got = device(ctx, case)
        ref = oracle(compiled, case)
        assert (got.stats.status == 0).all()
        assert_epochs_equal(got, ref)
        np.testing.assert_array_equal(got.stats.n_accepted, ref.stats.n_accepted)
        assert_vs_oracle(got, ref, what)
        assert_vs_reference(got, case, what)
    finally:
        ctx.close()
