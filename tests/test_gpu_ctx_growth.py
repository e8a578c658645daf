"""The blocks of a context that follow the batch (abi.cpp on nyx_amd/csrc/ctx_mem.h: a batch's arrays and their pinned mirror, the
STMs, the textbook form's stage matrices, the translated copy of a frame swap, the targeter's work and keep blocks) grow when a larger
batch comes: ONE context is handed a batch of 8, then one of 1 100 - past the floor of 1 024 elements and past a multiple of 64 -, then
the 8 again, and every result, states and stats, carries the bits a FRESH context returns for the same batch.  tuning.deterministic = 1,
under which tests/test_gpu_reproducible.py holds a context's bits to be independent of the batch.  A few steps each: seconds."""
import numpy as np
import pytest

import nyx_amd as nx
import target_cases as tc
from frame_swap_cases import MOON_FRAME, moon_batch
from frame_swap_cases import setup as swap_setup
from nyx_amd import _abi
from scenarios import dispersed_leo_batch, two_body_setup

pytestmark = pytest.mark.gpu

S = nx.NS_PER_S
SMALL, LARGE = 8, 1100
STATS = ("status", "last_step_ns", "last_error", "last_attempts", "n_accepted", "n_rejected", "n_evals")


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def two_body():
    prop, almanac, central = two_body_setup(nx.IntegratorMethod.RungeKutta89, nx.IntegratorOptions(), tc.MU)
    return prop.compile(almanac, central), dispersed_leo_batch(LARGE, seed=21), 300 * S


def stm_textbook():
    prop, almanac, central = two_body_setup(nx.IntegratorMethod.RungeKutta89, nx.IntegratorOptions.with_fixed_step_s(10.0), tc.MU)
    b = dispersed_leo_batch(LARGE, seed=22)
    b.reset_stm()
    return prop.compile(almanac, central, stm=True, stm_textbook=True), b, 50 * S


def frame_swap():
    prop, almanac, earth = swap_setup()
    return prop.compile(almanac, earth, state_frame=MOON_FRAME), moon_batch(LARGE, seed=23), 120 * S


def assert_same_run(got, want, label):
    (out, st), (ref, rst) = got, want
    np.testing.assert_array_equal(out.epoch_ns, ref.epoch_ns, err_msg=f"epoch_ns {label}")
    np.testing.assert_array_equal(out.step_ns, ref.step_ns, err_msg=f"step_ns {label}")
    for f in _abi.F64_FIELDS:
        np.testing.assert_array_equal(bits(getattr(out, f)), bits(getattr(ref, f)), err_msg=f"{f} {label}")
    if ref.stm is not None:
        np.testing.assert_array_equal(bits(out.stm), bits(ref.stm), err_msg=f"stm {label}")
    for f in STATS:
        a, b = getattr(st, f), getattr(rst, f)
        np.testing.assert_array_equal(bits(a) if a.dtype == np.float64 else a, bits(b) if b.dtype == np.float64 else b, err_msg=f"{f} {label}")


@pytest.mark.parametrize("case", [two_body, stm_textbook, frame_swap])
def test_a_grown_context_returns_a_fresh_contexts_bits(case):
    compiled, large, dur = case()
    batches = {SMALL: large.slice(0, SMALL), LARGE: large}
    tun = nx.Tuning(deterministic=1)
    fresh = {}
    for n, b in batches.items():
        ctx = nx.GpuContext(compiled, tuning=tun)
        fresh[n] = ctx.propagate(b, dur)
        ctx.close()
        out, st = fresh[n]
        assert (st.status == 0).all() and (st.n_accepted >= 2).all()
        assert not np.array_equal(out.rv(), b.rv())
    ctx = nx.GpuContext(compiled, tuning=tun)
    for k, n in enumerate((SMALL, LARGE, SMALL)):
        assert_same_run(ctx.propagate(batches[n], dur), fresh[n], f"(call {k}, n = {n})")
    ctx.close()


def assert_same_solution(got, want, label):
    for f in ("status", "iterations"):
        np.testing.assert_array_equal(getattr(got, f), getattr(want, f), err_msg=f"{f} {label}")
    assert got.iterations_run == want.iterations_run
    for f in ("correction", "achieved_errors"):
        np.testing.assert_array_equal(bits(getattr(got, f)), bits(getattr(want, f)), err_msg=f"{f} {label}")
    for states in ("corrected", "achieved"):
        a, b = getattr(got, states), getattr(want, states)
        np.testing.assert_array_equal(a.epoch_ns, b.epoch_ns, err_msg=f"{states}.epoch_ns {label}")
        for f in _abi.F64_FIELDS:
            np.testing.assert_array_equal(bits(getattr(a, f)), bits(getattr(b, f)), err_msg=f"{states}.{f} {label}")


def test_a_grown_context_targets_as_a_fresh_one():
    """nyx_hip_target_batch with 4 runs, then 1 100, then the 4 again: the work block of (1 + V) n rows and the keep block grow.
    The case: `sma_only`, the smallest of tests/target_cases.py that propagates (three variables, one objective, 2 iterations)."""
    c = tc.CASES["sma_only"]
    d = np.random.default_rng(24).normal(0.0, 1.0, (LARGE, 6)) * np.array([1.0, 1.0, 1.0, 1e-3, 1e-3, 1e-3])
    large = tc.batch_of(np.asarray(tc.RV0) + d, LARGE)
    batches = {4: large.slice(0, 4), LARGE: large}
    t0, t1 = tc.EPOCH, tc.EPOCH + c["dur_ns"]
    compiled, tun = tc.two_body_compiled(), nx.Tuning(deterministic=1)
    fresh = {}
    for n, b in batches.items():
        ctx = nx.GpuContext(compiled, tuning=tun)
        fresh[n] = ctx.target(b, c["variables"], c["objectives"], t0, t1)
        ctx.close()
        assert (fresh[n].status == 0).all() and (fresh[n].iterations >= 1).all()
    ctx = nx.GpuContext(compiled, tuning=tun)
    for k, n in enumerate((4, LARGE, 4)):
        assert_same_solution(ctx.target(batches[n], c["variables"], c["objectives"], t0, t1), fresh[n], f"(call {k}, n = {n})")
    ctx.close()
