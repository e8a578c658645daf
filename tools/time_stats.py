"""Times the ensemble statistics (include/nyx_hip_stats.h) at the headline shape: n runs x `seconds` of dense output, a sample every
`step_s`, eight `traj_values` rows, the 1 % / 50 % / 99 % band.  Two ways to the same numbers are timed, interleaved over `rounds`
rounds in ONE process after a warm-up round that is dropped:
  fused    `traj_values(.., stats=probs)`: the trajectories staged, the report and the reducer back to back on the device, only the
           statistics copied back (nyx_hip_traj_series_stats)
  numpy    what there was before: `traj_values` on the host (the whole values block copied back), then a vectorised numpy reduction
           (np.nanquantile, nanmin / nanmax / nanargmin / nanargmax, mean, sigma)
For each the wall time of the whole call and the device time of its kernel (`last_kernel_ms`: the reducer's launch after the fused
entry, the report's launch after `traj_values`) are printed, medians and extremes; staging the trajectories is common to both.  The
two results are compared before anything is timed.
usage: python tools/time_stats.py [n] [seconds] [step_s] [rounds]"""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np

import nyx_amd as nx
from nyx_amd.stats import STAT_FIXED, Stat
from scenarios import dispersed_leo_batch, leo_full_setup

n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000
seconds = int(sys.argv[2]) if len(sys.argv) > 2 else 5400
step_s = int(sys.argv[3]) if len(sys.argv) > 3 else 60
rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 7
probs = (0.01, 0.5, 0.99)
sp = nx.StateParameter
params = [sp.X, sp.Y, sp.Z, sp.Rmag, sp.Vmag, sp.SemiMajorAxis, sp.Eccentricity, sp.Inclination]
prop, almanac, central = leo_full_setup(degree=8)
ctx = nx.GpuContext(prop.compile(almanac, central))
dur, step = seconds * nx.NS_PER_S, step_s * nx.NS_PER_S
_, st, traj = ctx.propagate_with_traj(dispersed_leo_batch(n, seed=0), dur, capacity=seconds // 40 + 128)
assert (st.status == 0).all()
count = seconds // step_s + 1


def fused():
    stats, length = ctx.traj_values(traj, params, step, capacity=count, stats=probs)
    return stats, length, ctx.last_kernel_ms()


def numpy_way():
    values, length = ctx.traj_values(traj, params, step, capacity=count)
    ms = ctx.last_kernel_ms()
    out = np.empty((len(params), count, STAT_FIXED + len(probs)))
    out[:, :, STAT_FIXED:] = np.moveaxis(np.nanquantile(values, probs, axis=2), 0, -1)
    out[:, :, Stat.MIN], out[:, :, Stat.MAX] = np.nanmin(values, axis=2), np.nanmax(values, axis=2)
    out[:, :, Stat.ARGMIN], out[:, :, Stat.ARGMAX] = np.nanargmin(values, axis=2), np.nanargmax(values, axis=2)
    out[:, :, Stat.COUNT] = np.count_nonzero(~np.isnan(values), axis=2)
    out[:, :, Stat.SHIFT], out[:, :, Stat.SUM] = np.nanmean(values, axis=2), np.nanstd(values, axis=2, ddof=1)   # (mean and sigma in these two slots)
    return out, length, ms


# the same numbers both ways (the quantile formulas round differently: a few ulp)
a, la, _ = fused()
b, lb, _ = numpy_way()
assert (la == count).all() and (lb == count).all()
for c in (Stat.MIN, Stat.MAX, Stat.ARGMIN, Stat.ARGMAX, Stat.COUNT):
    assert (a[:, :, c] == b[:, :, c]).all(), c
assert np.allclose(a[:, :, STAT_FIXED:], b[:, :, STAT_FIXED:], rtol=1e-14, atol=0)
assert np.allclose(a[:, :, Stat.SHIFT] + a[:, :, Stat.SUM] / a[:, :, Stat.FINITE], b[:, :, Stat.SHIFT], rtol=1e-13, atol=0)

arms = {"fused": fused, "numpy": numpy_way}
wall, ms = {k: [] for k in arms}, {k: [] for k in arms}
for rep in range(rounds + 1):            # (round 0 warms every arm up and is dropped)
    for name, run in arms.items():
        t0 = time.perf_counter()
        _, _, kernel = run()
        t1 = time.perf_counter()
        if rep:
            wall[name].append((t1 - t0) * 1e3)
            ms[name].append(kernel)
rows = len(params)
print(f"{n} runs x {count} samples x {rows} rows, probs {probs}, {rounds} interleaved rounds after one warm-up; ms")
print(f"  values block {rows * count * n * 8 / 1e6:.1f} MB, statistics {rows * count * (STAT_FIXED + len(probs)) * 8 / 1e3:.1f} KB")
for name in arms:
    what = "reducer kernel" if name == "fused" else "report kernel "
    print(f"  {name:6s} wall median {np.median(wall[name]):9.2f}  min {min(wall[name]):9.2f}  max {max(wall[name]):9.2f}   "
          f"{what} median {np.median(ms[name]):7.3f}  min {min(ms[name]):7.3f}  max {max(ms[name]):7.3f}")
print(f"  reducer / report kernel = {np.median(ms['fused']) / np.median(ms['numpy']):.3f} (medians)")
print(f"  wall numpy / fused = {np.median(wall['numpy']) / np.median(wall['fused']):.2f} (medians), {min(wall['numpy']) / min(wall['fused']):.2f} (minima)")
ctx.close()
