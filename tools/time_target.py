"""Times the fused targeter loop (nyx_hip_target_batch, target_kernel.hip) against the same loop driven from the host, in one process:
  (a) two-body: `n` states dispersed about the 8000 km, e = 0.2 orbit (sigma 1 km, 1 m/s), Eccentricity -> 0.4 and SemiMajorAxis ->
      8100 km half a period later, three velocity variables (the case of tests/test_gpu_target.py)
  (b) the JWST point-mass configuration of the benchmarks: `n_jwst` dispersed states, Rmag one day later moved by 100 km
For each: the wall time of `GpuContext.target` (median of `reps` calls after a warm-up), the rounds it ran and the runs still active
per round; the kernel time of ONE propagation launch of the whole (1 + V) n work block (nyx_hip_last_kernel_ms of a plain
propagate_until_epoch of that many rows) times the rounds, as the share of the propagation launches when no run has ended; and the
host-driven loop (`targeter.target_definition` with `propagate_fn = ctx.propagate_until_epoch`) on `host_n` of the runs: its wall time
and the part of it spent inside `propagate_fn`, which is what the copies and the launches alone cost a host-driven loop.
usage: python tools/time_target.py [n] [n_jwst] [reps] [host_n]"""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np

import nyx_amd as nx
import target_cases as tc
from nyx_amd import _abi
from nyx_amd.frames import FrameParameter as FP, state_frame_value
from nyx_amd.targeter import Objective, target_definition
from scenarios import jwst_batch, jwst_setup

n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000
n_jwst = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
host_n = int(sys.argv[4]) if len(sys.argv) > 4 else 1000


def measure(label, ctx, batch, variables, objectives, t0, t1, mu):
    V = len(variables)
    call = lambda: ctx.target(batch, variables, objectives, t0, t1)   # noqa: E731
    sol = call()
    wall = []
    for _ in range(reps):
        s = time.perf_counter()
        sol = call()
        wall.append((time.perf_counter() - s) * 1e3)
    counts = np.bincount(sol.iterations, minlength=sol.iterations_run)
    active = batch.n - np.cumsum(counts)
    print(f"{label}: n = {batch.n}, fused wall {np.median(wall):.1f} ms, {sol.iterations_run} rounds, converged {sol.converged_fraction:.4f}, "
          f"active after each round {list(active)}", flush=True)
    # one propagation launch of the whole work block
    rows = np.tile(np.arange(batch.n), 1 + V)
    block = batch.take(rows)
    start, _ = ctx.propagate_until_epoch(block, t0)
    ctx.propagate_until_epoch(start, t1)
    ms = []
    for _ in range(reps):
        ctx.propagate_until_epoch(start, t1)
        ms.append(ctx.last_kernel_ms())
    k = float(np.median(ms))
    print(f"    one propagation launch of the {(1 + V) * batch.n} work rows: kernel {k:.2f} ms; x {sol.iterations_run} rounds = {k * sol.iterations_run:.1f} ms "
          f"= {k * sol.iterations_run / np.median(wall) * 100:.0f} % of the fused wall time were no run ever frozen", flush=True)
    # the host-driven loop on a part of the runs
    part = batch.slice(0, min(host_n, batch.n))
    inside = [0.0]

    def prop(b, end):
        s = time.perf_counter()
        out = ctx.propagate_until_epoch(b, end)
        inside[0] += time.perf_counter() - s
        return out
    s = time.perf_counter()
    want = target_definition(prop, part, variables, objectives, t0, t1, mu)
    host = (time.perf_counter() - s) * 1e3
    s = time.perf_counter()
    got = ctx.target(part, variables, objectives, t0, t1)
    fused = (time.perf_counter() - s) * 1e3
    same = np.array_equal(got.status, want.status) and np.array_equal(got.iterations, want.iterations)
    print(f"    host-driven loop, {part.n} runs: {host:.0f} ms, of which {inside[0] * 1e3:.0f} ms inside propagate_fn (copies and launches); fused on the same runs "
          f"{fused:.1f} ms; status and iterations equal: {same}", flush=True)


ctx = nx.GpuContext(tc.two_body_compiled(), tuning=nx.Tuning(deterministic=1))
c = tc.CASES["sma_ecc"]
rng = np.random.default_rng(5)
rv = np.asarray(tc.RV0) + np.concatenate([rng.normal(0.0, 1.0, (n, 3)), rng.normal(0.0, 1e-3, (n, 3))], axis=1)
measure("(a) two-body, Ecc and SMA", ctx, tc.batch_of(rv, n), c["variables"], c["objectives"], tc.EPOCH, tc.EPOCH + c["dur_ns"], tc.MU)
ctx.close()

prop, almanac, central = jwst_setup()
ctx = nx.GpuContext(prop.compile(almanac, central), tuning=nx.Tuning(deterministic=1))
batch = jwst_batch(n_jwst, seed=1)
t0 = int(batch.epoch_ns[0])
t1 = t0 + 86400 * nx.NS_PER_S
final, st = ctx.propagate_until_epoch(batch.slice(0, 1), t1)
mu = float(central.mu_km3_s2)
rmag = float(state_frame_value(FP.Rmag, final.rv(), mu)[0])
measure("(b) JWST point masses, Rmag + 100 km after a day", ctx, batch, tc.vel(), [Objective.within_tolerance(FP.Rmag, rmag + 100.0, 1.0)], t0, t1, mu)
ctx.close()
