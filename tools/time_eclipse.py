"""Times the fused eclipse launch against `traj_every` and the station-view launch on the same batch, in one process, on the
headline-sized ensemble (n trajectories x `hours` of dense output, one sample per `step_s`):
  (a) traj_every: the resampling alone, seven arrays per sample copied to the host
  (b) traj_eclipse, Sun / [Earth], [Occultation, State, BodyPenumbraMargin(Earth)]: resampled, the ephemerides evaluated at each
      sample's epoch, the disks overlapped, three arrays copied
  (c) traj_eclipse, Sun / [Earth, Moon], the same parameters: a second body = two more distinct segments and one more overlap
  (d) traj_eclipse, Sun / [Earth, Moon], [SunRange]: the interpolation and the ephemerides without asin / acos / the overlap
  (e) traj_aer, one station, [Azimuth, Elevation, Range, RangeRate]: the sibling report on the same batch
  (f) the host definition (eclipse.eclipse_value, the parameters of (c)) on the traj_every states of `host_runs` runs, timed once
      and scaled to n runs: what (a) still has to do on the host to produce what (c) returns; (a) + (f) is the route without the report
Kernel time is nyx_hip_last_kernel_ms, wall time is taken around the call; one warm-up call of each is excluded, the median of
`reps` timed calls is printed.  The force model is the 8x8 one of tools/time_traj.py: the dense output has the shape of the
headline's, the propagation is not what is timed here.
usage: python tools/time_eclipse.py [n] [hours] [step_s] [reps] [host_runs]"""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np

import nyx_amd as nx
from nyx_amd.eclipse import EclipseParameter as E
from nyx_amd.stations import AerParameter as A
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
sun, earth, moon = (almanac.frame_info(b) for b in (nx.SUN, nx.EARTH, nx.MOON))
ONE, TWO = nx.ShadowModel(sun, [earth]), nx.ShadowModel(sun, [earth, moon])
PARAMS = [E.Occultation, E.State, (E.BodyPenumbraMargin, 0)]
fixed = nx.Frame(central.naif_id, central.mu_km3_s2, 6378.1363, nx.IAU_EARTH_ROTATION, 1.0 / 298.257)
STATION = nx.GroundStation("Madrid", 40.427222, 4.250556, 0.834939, fixed, 5.0)


def timed(label, fn):
    fn()   # warm-up
    walls, kms = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        res = fn()
        walls.append(time.perf_counter() - t0)
        kms.append(ctx.last_kernel_ms())
    w, k = float(np.median(walls)), float(np.median(kms))
    print(f"{label:86s} wall {w * 1e3:9.1f} ms   kernel {k:8.2f} ms   (kernel min {min(kms):.2f}, max {max(kms):.2f})", flush=True)
    return w, k, res


wa, ka, ev = timed("(a) traj_every", lambda: ctx.traj_every(traj, step, count))
wb, kb, (vb, lb) = timed("(b) traj_eclipse, 1 body, [Occultation, State, BodyPenumbraMargin(Earth)]", lambda: ctx.traj_eclipse(traj, ONE, PARAMS, step, capacity=count))
assert (lb == ev.len).all()
print(f"    kernel (b) / (a): {kb / ka:.3f}   wall (b) / (a): {wb / wa:.3f}; bytes to the host {vb.nbytes + lb.nbytes} against {7 * 8 * count * n + 4 * n}", flush=True)
wc, kc, (vc, lc) = timed("(c) traj_eclipse, 2 bodies, the same parameters", lambda: ctx.traj_eclipse(traj, TWO, PARAMS, step, capacity=count))
print(f"    kernel (c) / (a): {kc / ka:.3f}   the second body: {kc - kb:.2f} ms kernel", flush=True)
rv = np.ascontiguousarray(ev.state[:, :count, :host_runs].transpose(1, 2, 0))
epochs = ev.epoch_ns[:count, :host_runs]
t0 = time.perf_counter()
want = [nx.eclipse_value(p[0] if isinstance(p, tuple) else p, rv, epochs, TWO, almanac, central, body=p[1] if isinstance(p, tuple) else None) for p in PARAMS]
wf = time.perf_counter() - t0
for p, w, got in zip(PARAMS, want, vc):
    name = p[0].name if isinstance(p, tuple) else p.name
    print(f"    {name:20s} largest |device - host definition| over {host_runs} runs: {np.abs(got[:, :host_runs] - w).max():.3e}", flush=True)
state = vc[1]
print(f"    share of the samples not fully lit: {(state != 0.0).mean():.4f}, in the umbra {(state == 2.0).mean():.4f}", flush=True)
print(f"(f) host definition, two bodies, three parameters: {wf * 1e3:.1f} ms for {host_runs} runs = {wf / host_runs * n:.1f} s scaled to {n} runs; "
      f"end to end (a) + (f) = {wa + wf / host_runs * n:.1f} s against {wc:.3f} s for (c) = {(wa + wf / host_runs * n) / wc:.0f} x", flush=True)
del vb, vc, ev, rv, want
wd, kd, _ = timed("(d) traj_eclipse, 2 bodies, [SunRange]: no asin, no acos, no overlap", lambda: ctx.traj_eclipse(traj, TWO, [E.SunRange], step, capacity=count)[1])
print(f"    the ephemerides of four distinct segments: {kd - ka:.2f} ms kernel over (a); asin / acos / overlap / parameters of (c): {kc - kd:.2f} ms", flush=True)
we, ke, _ = timed("(e) traj_aer, 1 station, [Azimuth, Elevation, Range, RangeRate]",
                  lambda: ctx.traj_aer(traj, [STATION], [A.Azimuth, A.Elevation, A.Range, A.RangeRate], step, capacity=count)[1])
print(f"    kernel (c) / (e): {kc / ke:.3f}", flush=True)
ctx.close()
