"""Times the link report against the RIC report on the same inputs: n runs x `seconds` of dense output, one transmitter (the nominal
flown retrograde), a sample every `step_s`.  Three launches are timed, interleaved over `rounds` rounds in ONE process: the link
report against the centre alone (no ephemeris segment evaluated), against the Earth and the Moon, and `traj_ric_diff` without its
median filter and moments (the same two interpolations per sample).  The figure is the device time of a whole launch
(`last_kernel_ms`: the init, the evaluation and the seal kernel; the first and the last are a few microseconds); a kernel trace
(`rocprofv3 --kernel-trace --stats -- python tools/time_link.py ...`, in a run of its own) splits it by kernel name
(`nyxlnk_values_kernel`, `nyxric_diff_kernel`).
usage: python tools/time_link.py [n] [seconds] [step_s] [rounds]"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np

import nyx_amd as nx
from nyx_amd.links import LinkParameter as L
from scenarios import dispersed_leo_batch, leo_full_setup, leo_nominal

n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000
seconds = int(sys.argv[2]) if len(sys.argv) > 2 else 5400
step_s = int(sys.argv[3]) if len(sys.argv) > 3 else 60
rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 7
prop, almanac, central = leo_full_setup(degree=8)
ctx = nx.GpuContext(prop.compile(almanac, central))
dur, step = seconds * nx.NS_PER_S, step_s * nx.NS_PER_S
cap = seconds // 40 + 128
_, st, traj = ctx.propagate_with_traj(dispersed_leo_batch(n, seed=0), dur, capacity=cap)
back = dispersed_leo_batch(1, seed=0)
back.set_rv((leo_nominal() * np.array([1.0, 1.0, 1.0, -1.0, -1.0, -1.0]))[None, :])
_, st_tx, tx = ctx.propagate_with_traj(back, dur, capacity=cap)
assert (st.status == 0).all() and (st_tx.status == 0).all()
count = seconds // step_s + 1
params = [L.Range, L.RangeRate, L.ReferenceDoppler, L.Visible, L.Clearance, L.LosX]   # six rows, as the RIC report writes
both = [central, almanac.frame_info(nx.MOON)]
arms = {"link, the centre": lambda: ctx.traj_link(traj, tx, params, step, capacity=count)[1],
        "link, Earth + Moon": lambda: ctx.traj_link(traj, tx, params, step, capacity=count, bodies=both)[1],
        "ric_diff": lambda: ctx.traj_ric_diff(traj, tx, step, capacity=count, smooth_window=0)[1]}
ms = {k: [] for k in arms}
for rep in range(rounds + 1):            # (round 0 warms every arm up and is dropped)
    for name, run in arms.items():
        length = run()
        assert (length == count).all(), (name, length.min(), length.max())
        if rep:
            ms[name].append(ctx.last_kernel_ms())
print(f"{n} runs x {count} samples, one transmitter, {rounds} interleaved rounds; device time of a launch, ms")
for name, v in ms.items():
    print(f"  {name:20s} median {np.median(v):8.3f}  min {min(v):8.3f}  max {max(v):8.3f}   = {n * count / np.median(v) / 1e3:.2f} M samples/s")
base = np.median(ms["ric_diff"])
for name in list(arms)[:2]:
    print(f"  ratio {name} / ric_diff = {np.median(ms[name]) / base:.3f} (medians), {min(ms[name]) / min(ms['ric_diff']):.3f} (minima)")
ctx.close()
