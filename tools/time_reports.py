"""Times the fused device reports against the path they replace, in one process, on the headline-sized ensemble
(n trajectories x `hours` of dense output, one sample per `step_s`):
  (a) today's path: traj_every + copy to host + state_value for SemiMajorAxis
  (b) traj_values (host flavour) for the same parameter
  (c) traj_values with four parameters against four runs of (a)
  (d) the windowed report on 256 runs: Results.values_of against Results.every_value_of_between (one launch per run)
Kernel time is nyx_hip_last_kernel_ms, wall time is taken around the call; one warm-up call of each is excluded, the
median of `reps` timed calls is printed.  The force model is the 8x8 one of tools/time_traj.py: the dense output has the
shape of the headline's, the propagation is not what is timed here.
usage: python tools/time_reports.py [n] [hours] [step_s] [reps]"""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np

import nyx_amd as nx
from nyx_amd.params import StateParameter as P, state_value
from scenarios import EPOCH0_NS, dispersed_leo_batch, leo_full_setup, leo_nominal

n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000
hours = float(sys.argv[2]) if len(sys.argv) > 2 else 24.0
step_s = float(sys.argv[3]) if len(sys.argv) > 3 else 60.0
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 3
prop, almanac, central = leo_full_setup(degree=8)
ctx = nx.GpuContext(prop.compile(almanac, central))
mu = central.mu_km3_s2
dur = int(hours * 3600) * nx.NS_PER_S
step = int(step_s * 1e9)
cap = int(hours * 3600 / 40) + 64
count = int(hours * 3600 / step_s) + 1
out, st, traj = ctx.propagate_with_traj(dispersed_leo_batch(n, seed=0), dur, capacity=cap)
print(f"ensemble: {n} x {hours:g} h, stored states max {traj.len.max()}, {count} samples per run every {step_s:g} s", flush=True)


def timed(label, fn, kernel=True):
    fn()   # warm-up
    walls, kms = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        res = fn()
        walls.append(time.perf_counter() - t0)
        kms.append(ctx.last_kernel_ms())
    w, k = float(np.median(walls)), float(np.median(kms))
    print(f"{label:64s} wall {w * 1e3:9.1f} ms" + (f"   kernel {k:8.2f} ms" if kernel else ""), flush=True)
    return w, k, res


def old_path(param):
    ev = ctx.traj_every(traj, step, count)
    return state_value(param, ev.state.transpose(1, 2, 0), mu)


FOUR = [P.SemiMajorAxis, P.Eccentricity, P.Inclination, P.Rmag]
wa, ka, va = timed("(a) traj_every + copy + state_value(SemiMajorAxis)", lambda: old_path(P.SemiMajorAxis))
wb, kb, (vb, lb) = timed("(b) traj_values([SemiMajorAxis])", lambda: ctx.traj_values(traj, [P.SemiMajorAxis], step, capacity=count))
print(f"    (b) / (a): wall {wb / wa:.3f}, kernel {kb / ka:.3f}; largest relative difference {np.nanmax(np.abs(vb[0] - va) / np.abs(va)):.2e}; "
      f"bytes to the host {vb.nbytes + lb.nbytes} against {7 * 8 * count * n + 4 * n}", flush=True)
wc4, kc4, _ = timed("(c) four runs of (a): SemiMajorAxis, Eccentricity, Inclination, Rmag", lambda: [old_path(p) for p in FOUR], kernel=False)
wc, kc, _ = timed("(c) traj_values(four parameters)", lambda: ctx.traj_values(traj, FOUR, step, capacity=count))
print(f"    (c) fused / four runs: wall {wc / wc4:.3f}; kernel of the fused launch {kc:.2f} ms against {ka:.2f} ms for ONE traj_every", flush=True)

# (d) windowed report on 256 runs
template = nx.Spacecraft(EPOCH0_NS, leo_nominal(), central, dry_mass_kg=100.0, srp_area_m2=1.0, cr=1.8)
mc = nx.MonteCarlo(nx.MvnSpacecraft.from_sigmas(template, [1.0, 1.0, 1.0, 1e-3, 1e-3, 1e-3]), seed=0)
res = mc.run_until_epoch(prop, almanac, EPOCH0_NS + dur, 256, capacity=cap)
ctx_mc = res._traj_ctx
lo, hi = EPOCH0_NS + dur // 4, EPOCH0_NS + 3 * (dur // 4)


def timed_mc(label, fn):
    fn()
    walls = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        walls.append(time.perf_counter() - t0)
    w = float(np.median(walls))
    print(f"{label:64s} wall {w * 1e3:9.1f} ms", flush=True)
    return w, r


wd0, listed = timed_mc("(d) every_value_of_between(SemiMajorAxis), 256 runs", lambda: res.every_value_of_between(P.SemiMajorAxis, step, lo, hi))
wd1, vs = timed_mc("(d) values_of([SemiMajorAxis]) on the same window", lambda: res.values_of([P.SemiMajorAxis], step, lo, hi))
flat = np.array(vs.flat(P.SemiMajorAxis))
print(f"    (d) fused / per-run: wall {wd1 / wd0:.4f}; {len(listed)} values, largest relative difference "
      f"{np.abs(flat - np.array(listed)).max() / np.abs(np.array(listed)).max():.2e}", flush=True)
ctx.close()
