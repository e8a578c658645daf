"""Times the fused ground-track launch against `traj_every` on the same batch, in one process, on the headline-sized
ensemble (n trajectories x `hours` of dense output, one sample per `step_s`):
  (a) traj_every: the resampling alone, seven arrays per sample copied to the host
  (b) traj_ground_track([Latitude, Longitude, Height, Rmag]) in IAU_EARTH: resampled, rotated, evaluated, four arrays copied
  (c) traj_ground_track([X .. VZ]) with frame.rotation None: the same launch without the frame block and the iteration
  (d) the host definition (groundtrack.ground_track_value, four parameters) on the traj_every states of `host_runs` runs,
      timed once and scaled to n runs: what (a) still has to do on the host to produce what (b) returns
Kernel time is nyx_hip_last_kernel_ms, wall time is taken around the call; one warm-up call of each is excluded, the
median of `reps` timed calls is printed.  The force model is the 8x8 one of tools/time_traj.py: the dense output has the
shape of the headline's, the propagation is not what is timed here.
usage: python tools/time_groundtrack.py [n] [hours] [step_s] [reps] [host_runs]"""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np

import nyx_amd as nx
from nyx_amd.groundtrack import GroundTrackParameter as G, ground_track_value
from scenarios import dispersed_leo_batch, leo_full_setup

n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000
hours = float(sys.argv[2]) if len(sys.argv) > 2 else 24.0
step_s = float(sys.argv[3]) if len(sys.argv) > 3 else 60.0
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 5
host_runs = min(n, int(sys.argv[5]) if len(sys.argv) > 5 else 64)
prop, almanac, central = leo_full_setup(degree=8)
ctx = nx.GpuContext(prop.compile(almanac, central))
dur = int(hours * 3600) * nx.NS_PER_S
step = int(step_s * 1e9)
cap = int(hours * 3600 / 40) + 64
count = int(hours * 3600 / step_s) + 1
out, st, traj = ctx.propagate_with_traj(dispersed_leo_batch(n, seed=0), dur, capacity=cap)
print(f"ensemble: {n} x {hours:g} h, stored states max {traj.len.max()}, {count} samples per run every {step_s:g} s", flush=True)
fixed = nx.Frame(central.naif_id, central.mu_km3_s2, 6378.1363, nx.IAU_EARTH_ROTATION, 1.0 / 298.257)
inertial = nx.Frame(central.naif_id, central.mu_km3_s2, 6378.1363, None, 1.0 / 298.257)
FOUR = [G.Latitude, G.Longitude, G.Height, G.Rmag]
CART = [G.X, G.Y, G.Z, G.VX, G.VY, G.VZ]


def timed(label, fn):
    fn()   # warm-up
    walls, kms = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        res = fn()
        walls.append(time.perf_counter() - t0)
        kms.append(ctx.last_kernel_ms())
    w, k = float(np.median(walls)), float(np.median(kms))
    print(f"{label:72s} wall {w * 1e3:9.1f} ms   kernel {k:8.2f} ms   (kernel min {min(kms):.2f}, max {max(kms):.2f})", flush=True)
    return w, k, res


wa, ka, ev = timed("(a) traj_every", lambda: ctx.traj_every(traj, step, count))
wb, kb, (vb, lb) = timed("(b) traj_ground_track([Latitude, Longitude, Height, Rmag]), IAU_EARTH", lambda: ctx.traj_ground_track(traj, fixed, FOUR, step, capacity=count))
wc, kc, (vc, lc) = timed("(c) traj_ground_track([X .. VZ]), no rotation", lambda: ctx.traj_ground_track(traj, inertial, CART, step, capacity=count))
print(f"    kernel (b) / (a): {kb / ka:.3f}   kernel (c) / (a): {kc / ka:.3f}   wall (b) / (a): {wb / wa:.3f}; "
      f"bytes to the host {vb.nbytes + lb.nbytes} against {7 * 8 * count * n + 4 * n}", flush=True)
assert (lb == ev.len).all() and (lc == ev.len).all()
assert np.array_equal(vc, ev.state[:, :count]), "the Cartesian values are not the traj_every states"
rv = np.ascontiguousarray(ev.state[:, :count, :host_runs].transpose(1, 2, 0))
epochs = ev.epoch_ns[:count, :host_runs]
t0 = time.perf_counter()
want = [ground_track_value(p, rv, epochs, fixed) for p in FOUR]
wd = time.perf_counter() - t0
for p, w, got in zip(FOUR, want, vb):
    print(f"    {p.name:10s} largest |device - host definition| over {host_runs} runs: {np.abs(got[:, :host_runs] - w).max():.3e}", flush=True)
print(f"(d) host definition, four parameters: {wd * 1e3:.1f} ms for {host_runs} runs = {wd / host_runs * n:.1f} s scaled to {n} runs, on top of (a)", flush=True)
ctx.close()
