"""The targeter cases the CPU and the GPU tests share (tests/test_target_host.py, tests/test_target_host_cxx.py,
tests/test_gpu_target.py): the 8000 km, e = 0.2 orbit of the reference's targeter tests with the achievement epoch half a period
later, the hyperbola of its B-plane test (b_plane.rs:30-37), and every deterministic input that ends in one of the status codes."""
import math

import numpy as np

import nyx_amd as nx
from nyx_amd import _abi, ephem
from nyx_amd.frames import FrameParameter as FP
from nyx_amd.targeter import Objective, TargetStatus, Variable, Vary
from scenarios import keplerian_to_cartesian, two_body_setup

MU = ephem.MU_EARTH
EPOCH = ephem.EPOCH_2024_02_29_NS
RV0 = keplerian_to_cartesian(8000.0, 0.2, 30.0, 60.0, 60.0, 0.0, MU)
HALF_PERIOD_NS = int(round(2.0 * math.pi * math.sqrt(8000.0 ** 3 / MU) / 2.0 * 1e9))
# b_plane.rs:30-37
RV_HYP = np.array([546507.344255845, -527978.380486028, 531109.066836708, -4.9220589268733, 5.36316523097915, -5.22166308425181])
# the reference's acceptance numbers (targeter tests conv_tgt_sma_ecc, tgt_b_plane_earth_gravity_assist_no_propagation)
GMAT_SMA_ECC_DV = 3.1160765514523914
GMAT_BPLANE_DV = 0.31909814507892165


def vel(max_step=0.2, guess=(0.0, 0.0, 0.0)):
    return [Variable(Vary.VelocityX, max_step=max_step, init_guess=guess[0]), Variable(Vary.VelocityY, max_step=max_step, init_guess=guess[1]),
            Variable(Vary.VelocityZ, max_step=max_step, init_guess=guess[2])]


def pos():
    return [Variable(Vary.PositionX), Variable(Vary.PositionY), Variable(Vary.PositionZ)]


SMA_ECC = [Objective.within_tolerance(FP.Eccentricity, 0.4, 1e-5), Objective.within_tolerance(FP.SemiMajorAxis, 8100.0, 0.1)]
BPLANE = [Objective.within_tolerance(FP.BdotT, 13135.7982982557, 1.0), Objective.within_tolerance(FP.BdotR, 5022.26511510685, 1.0)]

# name -> dict(rv, variables, objectives, dur_ns, frame, iterations, status, its (the prototype's count on the CPU oracle, or None))
CASES = {
    "sma_ecc": dict(rv=RV0, variables=vel(0.5), objectives=SMA_ECC, dur_ns=HALF_PERIOD_NS, status=TargetStatus.OK_CONVERGED, its=8),
    "bplane": dict(rv=RV_HYP, variables=vel(), objectives=BPLANE, dur_ns=0, status=TargetStatus.OK_CONVERGED, its=3),
    "singular": dict(rv=RV0, variables=vel(), objectives=[Objective.within_tolerance(FP.X, float(RV0[0]) + 1.0, 1e-3)], dur_ns=0,
                     status=TargetStatus.SINGULAR, its=0),
    "ineffective": dict(rv=RV0, variables=vel(0.0), objectives=SMA_ECC, dur_ns=HALF_PERIOD_NS, status=TargetStatus.INEFFECTIVE, its=1),
    "too_many": dict(rv=RV0, variables=vel(0.5), objectives=SMA_ECC, dur_ns=HALF_PERIOD_NS, iterations=3, status=TargetStatus.TOO_MANY_ITERATIONS, its=3),
    "not_finite": dict(rv=RV0, variables=vel(), objectives=[Objective.within_tolerance(FP.BdotT, 1000.0, 1.0)], dur_ns=HALF_PERIOD_NS,
                       status=TargetStatus.NOT_FINITE, its=0),
    "vnc": dict(rv=RV0, variables=vel(), objectives=SMA_ECC, dur_ns=HALF_PERIOD_NS, frame="VNC", status=TargetStatus.OK_CONVERGED, its=17),
    "delta_r": dict(rv=RV0, variables=pos(), objectives=[Objective.within_tolerance(FP.Rmag, 9700.0, 0.1)], dur_ns=HALF_PERIOD_NS,
                    status=TargetStatus.OK_CONVERGED, its=59),
    "sma_only": dict(rv=RV0, variables=vel(), objectives=[Objective.within_tolerance(FP.SemiMajorAxis, 8100.0, 0.1)], dur_ns=HALF_PERIOD_NS,
                     status=TargetStatus.OK_CONVERGED, its=2),
    "one_var_two_objs": dict(rv=RV0, variables=[Variable(Vary.VelocityY, max_step=0.5)],
                             objectives=[Objective.within_tolerance(FP.SemiMajorAxis, 8100.0, 0.1), Objective.within_tolerance(FP.Energy, -MU / (2.0 * 8100.0), 1e-4)],
                             dur_ns=HALF_PERIOD_NS, status=TargetStatus.OK_CONVERGED, its=2),
    "backward": dict(rv=RV0, variables=vel(0.5), objectives=SMA_ECC, dur_ns=-HALF_PERIOD_NS, status=TargetStatus.OK_CONVERGED, its=None),
    "guess": dict(rv=RV0, variables=vel(0.5, guess=(-0.8, 2.7, 1.0)), objectives=SMA_ECC, dur_ns=HALF_PERIOD_NS, status=TargetStatus.OK_CONVERGED, its=None),
}
# (measured on the CPU oracle by the prototype of the definition)
MEASURED_DV = {"sma_ecc": 3.06897, "bplane": 0.319557}


def two_body_compiled():
    prop, almanac, central = two_body_setup(nx.IntegratorMethod.RungeKutta89, nx.IntegratorOptions(), MU)
    return prop.compile(almanac, central)


def batch_of(rv, n=1, epoch_ns=EPOCH):
    b = _abi.StateBatch(n)
    b.set_rv(np.tile(np.asarray(rv, dtype=np.float64), (n, 1)) if np.ndim(rv) == 1 else rv)
    b.epoch_ns[:] = epoch_ns
    return b


def dispersed(n, seed=5, rv=RV0, sigma_r=1.0, sigma_v=1e-3):
    """n states about `rv` with sigma 1 km and 1 m/s, a fixed seed: row i is the same for every n."""
    rng = np.random.default_rng(seed)
    d = np.concatenate([rng.normal(0.0, sigma_r, (257, 3)), rng.normal(0.0, sigma_v, (257, 3))], axis=1)
    return batch_of(np.asarray(rv) + d[:n], n)


def oracle_until_epoch(compiled):
    """`propagate_fn` of targeter.target_definition on the CPU oracle: every row of a batch starts at the same epoch."""
    import oracle_lib

    def f(batch, end_epoch_ns):
        assert (batch.epoch_ns == batch.epoch_ns[0]).all()
        dur = int(end_epoch_ns) - int(batch.epoch_ns[0])
        if dur == 0:
            return batch.copy(), _abi.StatsBatch(batch.n)
        return oracle_lib.propagate(compiled, batch, dur)
    return f


def check_converged(sol, propagate_fn, batch, case, correction_epoch_ns, achievement_epoch_ns, mu=MU, about=None):
    """Item 4 of the issue: apply `correction` to xi_start independently, propagate, evaluate with frames.state_frame_value, and
    hold every |err_i| <= tol_i.  Needs no number.  `about(rv, epoch_ns)` translates to the objective frame."""
    from nyx_amd import frames
    from nyx_amd.targeter import _apply, _c6
    start, _ = propagate_fn(batch, correction_epoch_ns)
    xs = start.rv()
    vnc = case.get("frame") == "VNC"
    for i in np.flatnonzero(sol.converged):
        x = _apply(vnc, xs[i], _c6(case["variables"], sol.correction[:, i]), xs[i])
        assert np.array_equal(np.asarray(x), sol.corrected.rv()[i])
        one = start.slice(int(i), int(i) + 1)
        one.set_rv(np.asarray(x)[None, :])
        one.step_ns[:] = 0
        final, st = propagate_fn(one, achievement_epoch_ns)
        assert st.status[0] == 0
        rv = final.rv() if about is None else about(final.rv(), achievement_epoch_ns)
        for o in case["objectives"]:
            got = float(frames.state_frame_value(o.parameter, rv, mu)[0])
            err = o.multiplicative_factor * (o.desired_value - got) + o.additive_factor
            assert abs(err) <= o.tolerance, (o.parameter.name, err, o.tolerance)
