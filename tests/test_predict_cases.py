"""The references and scenarios of the device covariance-mapping tests (predict_cases.py), checked here on the CPU oracle: the
extended-precision time update against the oracle's double arithmetic, the process-noise selections, the run that fails in a later
segment, and the threaded front of the oracle."""
import numpy as np
import pytest

import nyx_amd as nx
import oracle_lib
import predict_cases as pc
from nyx_amd import _abi
from scenarios import EPOCH0_NS, leo_full_setup

S = nx.NS_PER_S


def oracle(compiled, case, noise=None):
    kw = pc.kwargs(case)
    if noise is not None:
        kw["process_noise"] = noise
    return oracle_lib.predict_until(compiled, case["batch"], case["p0"], case["end"], case["max_step"], **kw)


@pytest.mark.parametrize("frame", [None, "RIC", "VNC"])
@pytest.mark.parametrize("degree", [8, 0])
def test_time_update_reference_vs_oracle(degree, frame):
    """P-bar = Phi P Phi^T + Gamma Q Gamma^T recomputed in extended precision from the oracle's own Phi, epoch and nominal history
    (LEO, n = 40, six 60 s updates, decaying noise, inertial / RIC / VNC): the oracle's double arithmetic is within 1e-12 of it
    (measured maximum over the six cases: 2.6e-13 on P-bar, 2.8e-16 on the deviation), and the noise term is large enough to be seen at
    that bound: at least 1e-4 of every velocity diagonal element of P-bar (measured minimum: 1.5e-4, the inertial case; 1.3e-3 in RIC,
    2.2e-4 in VNC)."""
    prop, almanac, central = leo_full_setup(degree=degree)
    compiled = prop.compile(almanac, central, stm=True)
    case = pc.reference_case(frame)
    ref = oracle(compiled, case)
    n = case["batch"].n
    assert (ref.stats.status == 0).all() and (ref.n_updates == 6).all()
    e_p, e_d = pc.reference_errors(ref, case["p0"], case["batch"].epoch_ns, case["noise"], case["dev0"])
    share = np.inf
    for i in range(n):
        _, _, noise = pc.time_update_reference(case["p0"][i], ref.stm[:, i], ref.epochs_ns[:, i], ref.nominal[:, i], 6, case["batch"].epoch_ns[i],
                                               case["noise"], 6)
        d_noise, d_p = np.diagonal(noise, axis1=1, axis2=2)[:, 3:6], np.diagonal(ref.covar_history[:, i], axis1=1, axis2=2)[:, 3:6]
        share = min(share, (d_noise / d_p).min())
    print(f"degree {degree} {frame}: oracle vs extended precision Pbar {e_p:.2e} dev {e_d:.2e}, noise share of the velocity diagonal >= {share:.2e}")
    assert e_p <= 1e-12 and e_d <= 1e-12
    assert share >= 1e-4


def test_time_update_reference_backends_agree():
    """numpy's longdouble and mpmath at 50 digits give the same doubles but for the last bit (the longdouble result is rounded twice)."""
    pytest.importorskip("mpmath")
    prop, almanac, central = leo_full_setup(degree=0)
    compiled = prop.compile(almanac, central, stm=True)
    case = pc.reference_case("RIC", n=2)
    ref = oracle(compiled, case)
    args = (case["p0"][1], ref.stm[:, 1], ref.epochs_ns[:, 1], ref.nominal[:, 1], 6, case["batch"].epoch_ns[1], case["noise"], 6, case["dev0"][1])
    a, b = pc.time_update_reference(*args), pc.time_update_reference(*args, force_mpmath=True)
    assert pc.rel_err(a[0], b[0]) < 1e-15 and pc.dev_err(a[1], b[1]) < 1e-15
    np.testing.assert_allclose(a[2], b[2], rtol=1e-15, atol=0.0)
    assert np.abs(b[2]).max() > 0.0


@pytest.mark.parametrize("kind", ["disable", "late", "init_epoch"])
def test_noise_selection_cases_on_the_oracle(kind):
    """filtering.rs:64-80 on the oracle. 'disable': the last entry is passed over at every update (60 s > its 30 s disable time) and
    the run equals the first entry's alone bit for bit. 'late': the updates at 60 and 120 s equal the no-noise run's bits, those at 180
    and 240 s carry the noise. 'init_epoch': the decay clock starts 100 s before the batch. All within 1e-12 of the extended-precision
    recomputation (measured: 5.3e-14 on P-bar in each of the three, 2.1e-16 on the deviation)."""
    prop, almanac, central = leo_full_setup(degree=4)
    compiled = prop.compile(almanac, central, stm=True)
    case = pc.selection_case(kind)
    ref = oracle(compiled, case)
    assert (ref.stats.status == 0).all() and (ref.n_updates == 4).all()
    e_p, e_d = pc.reference_errors(ref, case["p0"], case["batch"].epoch_ns, case["noise"], case["dev0"])
    print(f"{kind}: oracle vs extended precision Pbar {e_p:.2e} dev {e_d:.2e}")
    assert e_p <= 1e-12 and e_d <= 1e-12
    none = oracle(compiled, case, noise=[])
    if case["twin"] is not None:
        twin = oracle(compiled, case, noise=case["twin"])
        u = case["twin_updates"]
        np.testing.assert_array_equal(ref.covar_history[u], twin.covar_history[u])
        np.testing.assert_array_equal(ref.stm, twin.stm)
    if kind == "disable":
        np.testing.assert_array_equal(ref.covar, twin.covar)
        assert (ref.covar_history[0, :, 3, 3] > none.covar_history[0, :, 3, 3]).all()         # the first entry does apply
        only_last = oracle(compiled, case, noise=case["noise"][1:])                          # and the last one alone never does
        np.testing.assert_array_equal(only_last.covar_history, none.covar_history)
    if kind == "late":
        assert (ref.covar_history[2, :, 3, 3] > none.covar_history[2, :, 3, 3]).all()
        # what the third update adds to the velocity diagonal is Gamma Q Gamma^T = dt^2 * q, on top of the no-noise run's value
        np.testing.assert_allclose(ref.covar_history[2, :, 3, 3] - none.covar_history[2, :, 3, 3], 60.0 ** 2 * 1e-11, rtol=1e-6)
    if kind == "init_epoch":
        plain = oracle(compiled, case, noise=[nx.ProcessNoise3D.with_decay(pc.REFERENCE_DIAG, 10 * 60 * S, pc.REFERENCE_DECAY)])
        got = ref.covar_history[0, :, 3, 3] - none.covar_history[0, :, 3, 3]
        own = plain.covar_history[0, :, 3, 3] - none.covar_history[0, :, 3, 3]
        np.testing.assert_allclose(got / own, np.exp(-pc.REFERENCE_DECAY[0] * 100.0), rtol=1e-6)


@pytest.mark.parametrize("degree", [0, 4])
def test_failure_in_a_later_segment_on_the_oracle(degree):
    """Runs that leave the almanac's coverage after one to three good updates, between runs that finish (RK4 at a fixed 10 s, 120 s
    segments, end = coverage end - 52 s).  The oracle, at both degrees: status [0, 4, 0, 4, 0, 4, 0, 4], n_updates
    [4, 1, 3, 2, 2, 0, 1, 3] for the eight start offsets, the failed runs stopped 2 s before the coverage end, six steps into their
    failing segment, their covariance the last good update's."""
    prop, almanac, central = pc.fixed_step_setup(degree)
    compiled = prop.compile(almanac, central, stm=True)
    case = pc.failure_case(almanac, 16)
    cov_end = pc.coverage_end_ns(almanac)
    assert abs((cov_end - EPOCH0_NS) / S / 86400.0 - 42.99) < 0.01
    for stages in pc.failure_stage_epochs(case):
        assert np.abs(stages - cov_end).min() > 1 * S
    ref = oracle(compiled, case)
    print(f"degree {degree}: status {ref.stats.status[:8].tolist()} n_updates {ref.n_updates[:8].tolist()}")
    assert list(ref.stats.status[:8]) == [0, 4, 0, 4, 0, 4, 0, 4] and list(ref.n_updates[:8]) == [4, 1, 3, 2, 2, 0, 1, 3]
    ok, failed = ref.stats.status == 0, ref.stats.status == _abi.ERR_EPHEM_RANGE
    assert (ok | failed).all()
    assert (ok & (ref.n_updates >= 3)).any()
    assert (failed & (ref.n_updates >= 1) & (ref.n_updates <= 3)).any()
    assert (failed & (ref.n_updates == 0)).any()
    assert (ref.states.epoch_ns[ok] == case["end"]).all()
    assert (ref.states.epoch_ns[failed] == cov_end - 2 * S).all()
    for i in np.flatnonzero(failed):
        u = ref.n_updates[i]
        np.testing.assert_array_equal(ref.covar[i], ref.covar_history[u - 1, i] if u else case["p0"][i])
        assert ref.stats.n_accepted[i] == 12 * u + 6


def test_oracle_predict_threaded_equals_the_serial_call():
    prop, almanac, central = leo_full_setup(degree=8)
    compiled = prop.compile(almanac, central, stm=True)
    n = 64
    b = pc.geo_batch(n, 5)
    p0, dev0 = pc.init_covar(n, 1), np.random.default_rng(1).standard_normal((n, 9)) * 1e-3
    kw = dict(process_noise=pc.loop_noise(), deviation_tracking=True, state_deviation=dev0, history=4)
    end = EPOCH0_NS + 240 * S
    a = oracle_lib.predict_until(compiled, b, p0, end, 60 * S, **kw)
    t = pc.oracle_predict_threaded(compiled, b, p0, end, 60 * S, **kw)
    assert (a.n_updates == 4).all()
    for f in ("covar", "state_deviation", "n_updates", "epochs_ns", "nominal", "stm", "covar_history", "deviation_history"):
        np.testing.assert_array_equal(getattr(t, f), getattr(a, f), err_msg=f)
    for f in ["epoch_ns", "stm", "step_ns"] + _abi.F64_FIELDS:
        np.testing.assert_array_equal(getattr(t.states, f), getattr(a.states, f), err_msg=f)
    for f in ("status", "last_step_ns", "last_error", "last_attempts", "n_accepted", "n_rejected", "n_evals"):
        np.testing.assert_array_equal(getattr(t.stats, f), getattr(a.stats, f), err_msg=f)
    # without history or deviations, and with fewer runs than threads
    a = oracle_lib.predict_until(compiled, b.slice(0, 3), p0[:3], end, 60 * S, history=2, keep_stm=False)
    t = pc.oracle_predict_threaded(compiled, b.slice(0, 3), p0[:3], end, 60 * S, history=2, keep_stm=False)
    assert t.stm is None
    np.testing.assert_array_equal(t.covar_history, a.covar_history)
    np.testing.assert_array_equal(t.covar, a.covar)
