"""The targeter's host definition (nyx_amd/targeter.py, `target_definition`) on the CPU oracle, two-body, RK89 defaults: the
reference's own acceptance numbers as its tests state them, every status code from one deterministic input, the frames, the clamp,
the under- and over-determined solves, and - for every converged case - the correction applied independently, propagated and
evaluated again (which needs no number).  No GPU."""
import math

import numpy as np
import pytest

import target_cases as tc
from nyx_amd import targeter
from nyx_amd.frames import FrameParameter as FP
from nyx_amd.targeter import Objective, TargetStatus, Variable, Vary, target_definition

_CACHE = {}


def prop():
    if "p" not in _CACHE:
        _CACHE["p"] = tc.oracle_until_epoch(tc.two_body_compiled())
    return _CACHE["p"]


def solve(name):
    """Each case is solved once and shared by the tests that look at it."""
    if name not in _CACHE:
        c = tc.CASES[name]
        b = tc.batch_of(c["rv"])
        _CACHE[name] = (target_definition(prop(), b, c["variables"], c["objectives"], tc.EPOCH, tc.EPOCH + c["dur_ns"], tc.MU,
                                          correction_frame=c.get("frame"), iterations=c.get("iterations", 100)), b)
    return _CACHE[name]


@pytest.mark.parametrize("name", sorted(tc.CASES))
def test_every_case_ends_as_stated(name):
    c = tc.CASES[name]
    sol, _ = solve(name)
    assert sol.status[0] == int(c["status"]), TargetStatus(int(sol.status[0])).name
    if c["its"] is not None:
        assert sol.iterations[0] == c["its"]
    assert sol.iterations_run == sol.iterations[0] + 1
    assert sol.converged_fraction == (1.0 if c["status"] == TargetStatus.OK_CONVERGED else 0.0)


@pytest.mark.parametrize("name", sorted(k for k, c in tc.CASES.items() if c["status"] == TargetStatus.OK_CONVERGED))
def test_converged_corrections_hold_when_flown_again(name):
    """Item 4 of the issue.  The `vnc` case is why the correction frame of a run is ONE frame, that of xi_start: with every step
    applied in the frame of the current xi, as the reference does, the total applied once missed Eccentricity 0.4 by 0.0723."""
    c = tc.CASES[name]
    sol, b = solve(name)
    tc.check_converged(sol, prop(), b, c, tc.EPOCH, tc.EPOCH + c["dur_ns"])
    # and the errors it reports are those of its own achieved state
    for i, o in enumerate(c["objectives"]):
        assert abs(sol.achieved_errors[i, 0]) <= o.tolerance


def test_reference_acceptance_sma_ecc():
    """conv_tgt_sma_ecc: converged, and |dv| below GMAT's or within 1e-6 of it."""
    sol, _ = solve("sma_ecc")
    dv = float(sol.delta_v_norm()[0])
    assert sol.status[0] == 0 and (dv < tc.GMAT_SMA_ECC_DV or abs(dv - tc.GMAT_SMA_ECC_DV) < 1e-6)
    assert abs(dv - tc.MEASURED_DV["sma_ecc"]) < 1e-4   # (the prototype's figure, five decimals)


def test_reference_acceptance_bplane_no_propagation():
    """tgt_b_plane_earth_gravity_assist_no_propagation: within 1e-3 km/s of GMAT's |dv|."""
    sol, _ = solve("bplane")
    dv = float(sol.delta_v_norm()[0])
    assert sol.status[0] == 0 and abs(dv - tc.GMAT_BPLANE_DV) < 1e-3
    assert abs(dv - tc.MEASURED_DV["bplane"]) < 1e-5


def test_vnc_correction_is_in_the_frame_of_the_start_state():
    sol, b = solve("vnc")
    print(f"vnc: {sol.iterations[0]} iterations, |dv| = {float(sol.delta_v_norm()[0]):.5f} km/s")
    # the inertial difference of the corrected state has the norm of the VNC correction (a rotation)
    d = sol.corrected.rv()[0] - b.rv()[0]
    assert np.array_equal(d[:3], np.zeros(3))
    assert abs(np.linalg.norm(d[3:]) - float(sol.delta_v_norm()[0])) < 1e-12


def test_max_step_clamps_the_step_not_the_total():
    sol, _ = solve("delta_r")
    # 59 rounds of at most 0.2 km per component: the total passes max_step many times over, no component passes 59 * 0.2
    assert np.abs(sol.correction[:, 0]).max() > 5.0 and np.abs(sol.correction[:, 0]).max() <= 59 * 0.2 + 1e-12


def test_statuses_keep_their_last_total_and_errors():
    sol, _ = solve("ineffective")
    assert np.array_equal(sol.correction[:, 0], np.zeros(3)) and np.isfinite(sol.achieved_errors[:, 0]).all()
    sol, _ = solve("not_finite")
    assert np.isnan(sol.achieved_errors[0, 0]) and np.array_equal(sol.correction[:, 0], np.zeros(3))
    sol, _ = solve("too_many")
    assert np.abs(sol.correction[:, 0]).max() > 0.0
    sol, _ = solve("guess")
    assert sol.status[0] == 0


def test_status_codes_are_the_headers():
    assert [int(s) for s in TargetStatus] == list(range(7))
    assert [s.name for s in TargetStatus] == ["OK_CONVERGED", "TOO_MANY_ITERATIONS", "INEFFECTIVE", "SINGULAR", "NOT_FINITE", "PROP_FAILED", "EPHEM_RANGE"]


def test_prop_failed_and_freezing_in_a_mixed_batch():
    """A propagation status other than 0 on one of a run's rows ends that run alone; the others go on as they do without it."""
    base = prop()

    def failing(batch, end_epoch_ns):
        out, st = base(batch, end_epoch_ns)
        st.status[np.isclose(batch.y_km, tc.RV0[1] + 7.0)] = 4   # the nominal row of run 1, every round
        return out, st
    c = tc.CASES["sma_ecc"]
    rv = np.tile(tc.RV0, (3, 1))
    rv[1, 1] += 7.0
    b = tc.batch_of(rv, 3)
    sol = target_definition(failing, b, c["variables"], c["objectives"], tc.EPOCH, tc.EPOCH + c["dur_ns"], tc.MU)
    one, _ = solve("sma_ecc")
    assert list(sol.status) == [0, int(TargetStatus.PROP_FAILED), 0] and sol.iterations[1] == 0 and np.isnan(sol.achieved_errors[:, 1]).all()
    for i in (0, 2):
        assert np.array_equal(sol.correction[:, i], one.correction[:, 0]) and sol.iterations[i] == one.iterations[0]
    assert sol.iterations_run == one.iterations_run


def test_cholesky_solve_against_numpy():
    rng = np.random.default_rng(2)
    for m in range(1, 7):
        a = rng.normal(size=(m, m + 2))
        g, b = a @ a.T, rng.normal(size=m)
        x = targeter.cholesky_solve(g.tolist(), b.tolist(), m)
        assert np.allclose(x, np.linalg.solve(g, b), rtol=1e-9, atol=1e-12)
    assert targeter.cholesky_solve([[0.0]], [1.0], 1) is None
    assert targeter.cholesky_solve([[1.0, 0.0], [2.0, 1.0]], [1.0, 1.0], 2) is None        # not positive definite: the second pivot is -3
    assert targeter.cholesky_solve([[math.inf]], [1.0], 1) is None


def test_refusals_of_the_problem():
    v, o = tc.vel(), tc.SMA_ECC
    with pytest.raises(ValueError, match="n_vars = 0"):
        targeter.check_problem([], o, None, 100)
    with pytest.raises(ValueError, match="n_objs = 8"):
        targeter.check_problem(v, o * 4, None, 100)
    with pytest.raises(ValueError, match="iterations = 1001"):
        targeter.check_problem(v, o, None, 1001)
    with pytest.raises(ValueError, match="var_perturbation\\[1\\]"):
        targeter.check_problem([v[0], Variable(Vary.VelocityY, perturbation=0.0)], o, None, 100)
    with pytest.raises(ValueError, match="var_max_step\\[0\\]"):
        targeter.check_problem([Variable(Vary.VelocityY, max_step=-1.0)], o, None, 100)
    with pytest.raises(ValueError, match="var_min_value\\[0\\]"):
        targeter.check_problem([Variable(Vary.VelocityY, min_value=6.0)], o, None, 100)
    with pytest.raises(ValueError, match="obj_tolerance\\[0\\]"):
        targeter.check_problem(v, [Objective.within_tolerance(FP.X, 1.0, -1.0)], None, 100)
    with pytest.raises(ValueError, match="is a position"):
        targeter.check_problem(tc.pos(), o, "VNC", 100)
    with pytest.raises(ValueError, match="correction_frame"):
        targeter.check_problem(v, o, "RIC", 100)


def test_bplane_target_objectives():
    objs = targeter.BPlaneTarget.from_bt_br(13135.7982982557, 5022.26511510685).to_objectives()
    assert {o.parameter for o in objs} == {FP.BdotT, FP.BdotR} and all(o.tolerance == 1.0 for o in objs)
