"""Times the Lambert kernels (lambert_kernel.hip) in one process:
  (a) lambert_grid, Earth -> Jupiter barycentre about the Sun, `side` x `side` cells (default 1024 x 1024) on the 40-day almanac of the
      tests, arrivals by epoch, [C3, VinfArr, DlaDeg, TofS]: the tile's body states evaluated once and parked, one solve per lane
  (b) the same grid with arrivals by time of flight: every lane evaluates its own arrival state
  (c) lambert_batch, `n` seeded problems about the Earth (default 10^6), the same four parameters
  (d) the host definition (lambert.solve) on `host_n` of the problems of (c), timed once: seconds per solve of the Python restatement
Kernel time is nyx_hip_last_kernel_ms, wall time is taken around the call (it includes the copies of the host flavour); one warm-up
call of each is excluded, the median of `reps` timed calls is printed with the solves per second of the kernel.
usage: python tools/time_lambert.py [side] [n] [reps] [host_n]"""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np

import nyx_amd as nx
from nyx_amd import lambert
from nyx_amd.lambert import LambertParameter as P
from scenarios import EPOCH0_NS, leo_full_setup

side = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
n = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
host_n = min(n, int(sys.argv[4]) if len(sys.argv) > 4 else 2000)
DAY = 86400 * nx.NS_PER_S
PARAMS = [P.C3, P.VinfArr, P.DlaDeg, P.TofS]
prop, almanac, central = leo_full_setup(degree=0)
ctx = nx.GpuContext(prop.compile(almanac, central))
earth, jupiter, sun = (almanac.frame_info(b) for b in (central.naif_id, nx.JUPITER_BARYCENTER, nx.SUN))


def timed(label, solves, call):
    call()
    ms, wall = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = call()
        wall.append((time.perf_counter() - t0) * 1e3)
        ms.append(ctx.last_kernel_ms())
    k = float(np.median(ms))
    print(f"{label}: kernel {k:.3f} ms, {solves / k * 1e3:.3e} solves/s, wall {np.median(wall):.1f} ms, solved {out.feasible_fraction:.3f}", flush=True)
    return out


dep_step, arr_step = 8 * DAY // side, 28 * DAY // side
timed(f"(a) grid {side} x {side} by epoch", side * side,
      lambda: ctx.lambert_grid(earth, jupiter, sun, PARAMS, side, side, EPOCH0_NS, dep_step, arr0_ns=EPOCH0_NS + 10 * DAY, arr_step_ns=arr_step))
timed(f"(b) grid {side} x {side} by time of flight", side * side,
      lambda: ctx.lambert_grid(earth, jupiter, sun, PARAMS, side, side, EPOCH0_NS, dep_step, tof0_ns=4 * DAY, tof_step_ns=arr_step))
rng = np.random.default_rng(0)
d1, d2 = rng.normal(size=(n, 3)), rng.normal(size=(n, 3))
rv1 = np.concatenate([d1 / np.linalg.norm(d1, axis=1)[:, None] * rng.uniform(7000.0, 42000.0, size=(n, 1)), rng.normal(size=(n, 3))], axis=1).T.copy()
rv2 = np.concatenate([d2 / np.linalg.norm(d2, axis=1)[:, None] * rng.uniform(7000.0, 42000.0, size=(n, 1)), rng.normal(size=(n, 3))], axis=1).T.copy()
tof = 10.0 ** rng.uniform(3.3, 5.5, size=n)
mu = float(earth.mu_km3_s2)
for m in (0, 1):
    got = timed(f"(c) batch {n}, n_revs = {m}", n, lambda: ctx.lambert_batch(rv1, rv2, tof, mu, PARAMS + [P.Iterations], n_revs=m))
    it = got.of(P.Iterations)
    print(f"    Householder steps: min {np.nanmin(it):.0f}, mean {np.nanmean(it):.2f}, max {np.nanmax(it):.0f}", flush=True)
t0 = time.perf_counter()
for i in range(host_n):
    lambert.solve(rv1[:, i], rv2[:, i], tof[i], mu)
print(f"(d) host definition (Python): {(time.perf_counter() - t0) / host_n * 1e6:.1f} us per solve")
