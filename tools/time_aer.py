"""Times the fused station-view launch against `traj_every` on the same batch, in one process, on the headline-sized
ensemble (n trajectories x `hours` of dense output, one sample per `step_s`):
  (a) traj_every: the resampling alone, seven arrays per sample copied to the host
  (b) traj_aer, 1 station, [Azimuth, Elevation, Range, RangeRate]: resampled, rotated, evaluated, four arrays copied
  (c) traj_aer, 4 stations, [Azimuth, Elevation, Range] in ONE launch: one interpolation and one rotation per sample serve all four
  (d) the four stations of (c) in four single-station launches: kernel times added
  (e) 4 stations, [RhoS, RhoE, RhoZ]: (c) without asin / atan2 - what the transcendental part of a station costs
  (f) the host definition (stations.aer_value, the parameters of (b)) on the traj_every states of `host_runs` runs, timed once and
      scaled to n runs: what (a) still has to do on the host, PER STATION, to produce what (b) returns
The cost of a further station is (t_c - t_1) / 3 with t_1 = one station with the parameters of (c).  Kernel time is
nyx_hip_last_kernel_ms, wall time is taken around the call; one warm-up call of each is excluded, the median of `reps` timed calls is
printed.  The force model is the 8x8 one of tools/time_traj.py: the dense output has the shape of the headline's, the propagation is
not what is timed here.
usage: python tools/time_aer.py [n] [hours] [step_s] [reps] [host_runs]"""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np

import nyx_amd as nx
from nyx_amd.stations import AerParameter as A, aer_value
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
STATIONS = [nx.GroundStation("Madrid", 40.427222, 4.250556, 0.834939, fixed, 5.0), nx.GroundStation("Canberra", -35.398333, 148.981944, 0.691750, fixed, 5.0),
            nx.GroundStation("Goldstone", 35.247164, 243.205, 1.07114904, fixed, 5.0), nx.GroundStation("Kiruna", 67.857, 20.964, 0.402, fixed, 10.0)]
FOUR = [A.Azimuth, A.Elevation, A.Range, A.RangeRate]
THREE = [A.Azimuth, A.Elevation, A.Range]
RHO = [A.RhoS, A.RhoE, A.RhoZ]


def timed(label, fn):
    fn()   # warm-up
    walls, kms = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        res = fn()
        walls.append(time.perf_counter() - t0)
        kms.append(ctx.last_kernel_ms())
    w, k = float(np.median(walls)), float(np.median(kms))
    print(f"{label:78s} wall {w * 1e3:9.1f} ms   kernel {k:8.2f} ms   (kernel min {min(kms):.2f}, max {max(kms):.2f})", flush=True)
    return w, k, res


wa, ka, ev = timed("(a) traj_every", lambda: ctx.traj_every(traj, step, count))
wb, kb, (vb, lb) = timed("(b) traj_aer, 1 station, [Azimuth, Elevation, Range, RangeRate]", lambda: ctx.traj_aer(traj, STATIONS[:1], FOUR, step, capacity=count))
assert (lb == ev.len).all()
print(f"    kernel (b) / (a): {kb / ka:.3f}   wall (b) / (a): {wb / wa:.3f}; bytes to the host {vb.nbytes + lb.nbytes} against {7 * 8 * count * n + 4 * n}", flush=True)
rv = np.ascontiguousarray(ev.state[:, :count, :host_runs].transpose(1, 2, 0))
epochs = ev.epoch_ns[:count, :host_runs]
t0 = time.perf_counter()
want = [aer_value(p, rv, epochs, STATIONS[0]) for p in FOUR]
wf = time.perf_counter() - t0
for p, w, got in zip(FOUR, want, vb[0]):
    d = got[:, :host_runs] - w
    d = (d + 180.0) % 360.0 - 180.0 if p is A.Azimuth else d
    print(f"    {p.name:10s} largest |device - host definition| over {host_runs} runs: {np.abs(d).max():.3e}", flush=True)
print(f"(f) host definition, one station, four parameters: {wf * 1e3:.1f} ms for {host_runs} runs = {wf / host_runs * n:.1f} s scaled to {n} runs, "
      f"on top of (a), per station", flush=True)
del vb, ev, rv, want
wc, kc, (vc, lc) = timed("(c) traj_aer, 4 stations, [Azimuth, Elevation, Range], one launch", lambda: ctx.traj_aer(traj, STATIONS, THREE, step, capacity=count))
print(f"    output of (c): {vc.nbytes} bytes = {vc.nbytes / 1e9:.3f} GB", flush=True)
singles = []
for s, station in enumerate(STATIONS):
    w1, k1, (v1, l1) = timed(f"(d) traj_aer, 1 station ({station.name}), [Azimuth, Elevation, Range]", lambda: ctx.traj_aer(traj, [station], THREE, step, capacity=count))
    assert np.array_equal(v1[0], vc[s], equal_nan=True), "a station alone is not its row of the four-station launch"
    singles.append((w1, k1))
    del v1
del vc
k1 = float(np.median([k for _, k in singles]))
print(f"    a further station: (t4 - t1) / 3 = ({kc:.2f} - {k1:.2f}) / 3 = {(kc - k1) / 3:.2f} ms kernel = {(kc - k1) / 3 / k1:.3f} of a one-station launch; "
      f"four single launches {sum(k for _, k in singles):.2f} ms kernel against {kc:.2f} ms in one = {sum(k for _, k in singles) / kc:.2f} x; "
      f"wall {sum(w for w, _ in singles) * 1e3:.1f} ms against {wc * 1e3:.1f} ms", flush=True)
we, ke, _ = timed("(e) traj_aer, 4 stations, [RhoS, RhoE, RhoZ]: no asin, no atan2", lambda: ctx.traj_aer(traj, STATIONS, RHO, step, capacity=count)[1])
print(f"    asin + atan2 of four stations: {kc - ke:.2f} ms kernel of {kc:.2f}", flush=True)
ctx.close()
