"""Times the fused RIC dispersions against the composition they replace, in one process, on the same trajectories
(n runs x `hours` of dense output and one nominal, one sample per `step_s`):
  (a') the composition without the filter: two traj_every launches (the runs, the nominal) + the copy back of their
       states + ric_difference + numpy sums of the moments
  (a)  (a') + smooth_ric of every run (a Python loop, seconds at this size: timed ONCE, host only, and reported separately
       so that it does not hide the rest)
  (b) traj_ric_diff with the values and the moments (6 K n + 28 K doubles back)
  (c) traj_ric_diff_device on device-resident trajectories, only the 28 K moments copied back
Kernel time is nyx_hip_last_kernel_ms, wall time is taken around the call (every path ends in a device synchronise); one
warm-up call of each is excluded, the median and the spread of `reps` timed calls are printed, the paths alternate.
(a') is also printed in its two parts: the traj_every calls (with their kernel time) and the numpy work.
The force model is the 8x8 one of tools/time_traj.py: the propagation is not what is timed here.
usage: python tools/time_ric.py [n] [hours] [step_s] [reps]"""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np

import nyx_amd as nx
from nyx_amd import _abi
from nyx_amd.mc import ric_moments
from nyx_amd.params import ric_difference, smooth_ric
from scenarios import dispersed_leo_batch, leo_full_setup, leo_nominal

n = int(sys.argv[1]) if len(sys.argv) > 1 else 5_000
hours = float(sys.argv[2]) if len(sys.argv) > 2 else 24.0
step_s = float(sys.argv[3]) if len(sys.argv) > 3 else 60.0
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 5
prop, almanac, central = leo_full_setup(degree=8)
ctx = nx.GpuContext(prop.compile(almanac, central))
dur = int(hours * 3600) * nx.NS_PER_S
step = int(step_s * 1e9)
cap = int(hours * 3600 / 40) + 64
count = int(hours * 3600 / step_s) + 1
out, st, traj = ctx.propagate_with_traj(dispersed_leo_batch(n, seed=0), dur, capacity=cap)
nominal = dispersed_leo_batch(1, seed=0)
nominal.set_rv(leo_nominal()[None, :])
_, st1, nom = ctx.propagate_with_traj(nominal, dur, capacity=cap)
assert (st.status == 0).all() and (st1.status == 0).all()
print(f"ensemble: {n} x {hours:g} h and one nominal, stored states max {traj.len.max()}, {count} samples per run every {step_s:g} s", flush=True)


stages = []   # of every call of the composition: (wall of the two traj_every calls, their kernel ms, wall of the numpy part)


def composition():
    t0 = time.perf_counter()
    ev = ctx.traj_every(traj, step, count)
    kernel_ms = ctx.last_kernel_ms()
    evn = ctx.traj_every(nom, step, count)
    kernel_ms += ctx.last_kernel_ms()
    t1 = time.perf_counter()
    d = ric_difference(ev.state.transpose(1, 2, 0), evn.state.transpose(1, 2, 0))          # [K, n, 6]
    cols = [d[:, i].T for i in range(n)]
    mom = ric_moments(cols, count)
    stages.append((t1 - t0, kernel_ms, time.perf_counter() - t1))
    return cols, mom


def fused():
    return ctx.traj_ric_diff(traj, nom, step, capacity=count, smooth_window=5, moments=True)


def device_resident():
    import torch
    dev = torch.device("cuda", 0)
    keep = []

    def on_device(t):
        epoch, state, tlen = torch.from_numpy(t.epoch_ns).to(dev), torch.from_numpy(t.state).to(dev), torch.from_numpy(t.len).to(dev)
        keep.extend([epoch, state, tlen])
        s = _abi.Traj()
        s.capacity = t.capacity
        s.epoch_ns = C.cast(epoch.data_ptr(), _abi.c_int64_p)
        for k, f in enumerate(["x_km", "y_km", "z_km", "vx_km_s", "vy_km_s", "vz_km_s"]):
            setattr(s, f, C.cast(state[k].data_ptr(), _abi.c_double_p))
        s.len = C.cast(tlen.data_ptr(), _abi.c_int32_p)
        return s

    s, r = on_device(traj), on_device(nom)
    values = torch.empty(6 * count * n, dtype=torch.float64, device=dev)
    length = torch.empty(n, dtype=torch.int32, device=dev)
    mom = torch.empty(count * 28, dtype=torch.float64, device=dev)
    q = _abi.RicQuery()
    q.step_ns, q.frame_of, q.transport, q.smooth_window = step, 1, 1, 5
    lib = _abi.load_library()

    def call():
        rc = lib.nyx_hip_traj_ric_diff_device(ctx._h, C.byref(s), n, C.byref(r), 1, C.byref(q), count, C.c_void_p(values.data_ptr()),
                                              C.c_void_p(length.data_ptr()), None, C.c_void_p(mom.data_ptr()), None)
        assert rc == 0, _abi.last_error()
        return mom.cpu().numpy().reshape(count, 28)       # (the copy synchronises)

    return call, keep


paths = [("(a') two traj_every + copy + ric_difference + numpy sums", composition, False),
         ("(b) traj_ric_diff: values + moments to the host", fused, True)]
dev_call, _keep = device_resident()
paths.append(("(c) traj_ric_diff_device: resident input, moments to the host", dev_call, True))
results, walls, kms = {}, {p[0]: [] for p in paths}, {p[0]: [] for p in paths}
for label, fn, _ in paths:
    fn()   # warm-up
for _ in range(reps):
    for label, fn, kernel in paths:
        t0 = time.perf_counter()
        results[label] = fn()
        walls[label].append(time.perf_counter() - t0)
        kms[label].append(ctx.last_kernel_ms() if kernel else float("nan"))
for label, _, kernel in paths:
    w = np.array(walls[label]) * 1e3
    print(f"{label:74s} wall {np.median(w):10.1f} ms (min {w.min():.1f}, max {w.max():.1f})" + (f"   kernels {np.median(kms[label]):8.2f} ms" if kernel else ""),
          flush=True)
every_s, every_kms, host_s = (np.array(c) for c in zip(*stages[1:]))   # (without the warm-up call)
print(f"of (a'): the two traj_every calls {np.median(every_s) * 1e3:.1f} ms wall (min {every_s.min() * 1e3:.1f}, max {every_s.max() * 1e3:.1f}), "
      f"their kernels {np.median(every_kms):.2f} ms; ric_difference + numpy sums {np.median(host_s) * 1e3:.1f} ms "
      f"(min {host_s.min() * 1e3:.1f}, max {host_s.max() * 1e3:.1f})", flush=True)
raw_cols, _ = results[paths[0][0]]
t0 = time.perf_counter()
cols = [smooth_ric(c.T, 5).T for c in raw_cols]
mom_a = ric_moments(cols, count)
t_smooth = time.perf_counter() - t0
print(f"smooth_ric of {n} runs + the sums of the filtered columns, on the host, once: {t_smooth * 1e3:.1f} ms", flush=True)
vals, length, epoch0, mom_b = results[paths[1][0]]
mom_c = results[paths[2][0]]
same = all(np.array_equal(vals[:, :, i], cols[i]) for i in range(n))
rel = np.max(np.abs(mom_b[:, 7:] - mom_a[:, 7:]) / np.maximum(np.abs(mom_a[:, 7:]), 1e-300))
print(f"values of (b) equal to (a) bit for bit: {same}; moments (b) == (c) bit for bit: {np.array_equal(mom_b, mom_c)}; counts (a) == (b): "
      f"{np.array_equal(mom_a[:, 0], mom_b[:, 0])}; largest relative difference of the second moments (a) - (b): {rel:.2e}")
print(f"samples per run: {int(length.min())} .. {int(length.max())} of {count}")
# what traj_every returns is a TrajBatch: the epoch and the six states of every sample, and len; the nominal is ONE
# trajectory here, so the composition copies 7 K (n + 1) words, not the 12 K n doubles of two full batches of states
print(f"bytes to the host: (a) {7 * 8 * count * (n + 1) + 4 * (n + 1)} (epochs + 6 states of every sample of the runs and the nominal; "
      f"the states alone {6 * 8 * count * (n + 1)}), (b) {vals.nbytes + length.nbytes + epoch0.nbytes + mom_b.nbytes}, (c) {mom_c.nbytes}", flush=True)
wa2, wb, wc = (float(np.median(walls[paths[k][0]])) for k in (0, 1, 2))
print(f"(b) / (a'): {wb / wa2:.4f}   (c) / (a'): {wc / wa2:.4f}   (b) / (a = a' + filter): {wb / (wa2 + t_smooth):.4f}", flush=True)
ctx.close()
