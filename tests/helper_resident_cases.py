"""The GPU cases of tests/test_gpu_helper_resident.py, one per process: `python helper_resident_cases.py CASE` propagates the case's
ensemble twice - `Tuning.helper_resident` = 1 and 0, everything else alike - compares states and statistics bit for bit and prints one
JSON line.  A process per case so that the test can put each GPU step under a time limit of its own."""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import nyx_amd as nx  # noqa: E402
import scenarios as sc  # noqa: E402

NO_FAN = 0x8000000    # small ensembles in the claim mode: the resident feed is the claim-mode helpers'
ONE_PART = 0x80000    # one-part hand-off whatever the field (and no fan-out mode)

# name: (field, degree, trajectories, minutes, tuning besides helper_resident)
CASES = {
    # degree 70, sixteen waves, 1 h, cooperative mode forced; 700 = 11 owners, the last one part-filled, 11 claim-mode helpers whose fast
    # waves walk two columns each
    "deg70_n700": ("earth", 70, 700, 60, dict(cooperative=1, debug_flags=NO_FAN)),
    # a single owner cannot have resident helpers: the claim mode wants at least eight helpers and at most three per owner
    # (plan_cooperation), so one owner cooperates in the fan-out mode, whose kernel keeps its feed - both runs walk with the old one
    "deg70_n64": ("earth", 70, 64, 60, dict(cooperative=1)),
    # the smallest claim-mode launch: three owners, three helpers each (nine workgroups stage the rows for three mailboxes)
    "deg70_n192": ("earth", 70, 192, 60, dict(cooperative=1, coop_helper_ratio=3.0)),
    # helper columns of 28 .. 41 rows, no multiple of a group; and of 12 .. 25, some shorter than one group
    "deg40_n520": ("earth", 40, 520, 60, dict(cooperative=1, debug_flags=NO_FAN)),
    "deg24_n520": ("earth", 24, 520, 60, dict(cooperative=1, debug_flags=NO_FAN)),
    # helpers that never answer: every owner walks the helper's columns itself once and finishes alone
    "fallback_deg70_n700": ("earth", 70, 700, 60, dict(cooperative=1, debug_flags=NO_FAN, coop_mute=1)),
    # blocks that do not fit: 150x150 with no helpers at all at 128 trajectories, and with a one-part hand-off at 512 (168 KB of rows)
    "nofit_deg150_n128": ("moon", 150, 128, 10, dict(cooperative=1)),
    "nofit_deg150_n512": ("moon", 150, 512, 10, dict(cooperative=1, debug_flags=ONE_PART)),
}


def run(case):
    field, degree, n, minutes, tuning = CASES[case]
    if field == "earth":
        prop, almanac, central = sc.leo_full_setup(degree=degree)
        batch = sc.dispersed_leo_batch(n, seed=23)
    else:
        prop, almanac, central = sc.lunar_setup(degree=degree)
        batch = sc.lunar_batch(n, seed=23)
    compiled = prop.compile(almanac, central)
    dur = minutes * 60 * nx.NS_PER_S
    res = {}
    for resident in (1, 0):
        ctx = nx.GpuContext(compiled, tuning=nx.Tuning(helper_resident=resident, **tuning))
        out, st = ctx.propagate(batch, dur)
        res[resident] = dict(rv=out.rv().copy(), epoch=out.epoch_ns.copy(), status=st.status.copy(), acc=st.n_accepted.copy(),
                             rej=st.n_rejected.copy(), evals=st.n_evals.copy(), helpers=ctx.last_coop_helpers(), feed=ctx.last_helper_feed(),
                             ms=ctx.last_kernel_ms())
        ctx.close()
    # the device's own word: the accounting twin of the kernel counts the helper jobs and, among them, those walked from LDS
    jobs, lds_jobs, twin_equal = [], [], []
    for resident in (1, 0):
        ctx = nx.GpuContext(compiled, tuning=nx.Tuning(helper_resident=resident, profile=1, **tuning))
        out, st = ctx.propagate(batch, dur)
        buf = (C.c_int64 * 136)()
        ctx._lib.nyx_hip_debug_profile.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        assert ctx._lib.nyx_hip_debug_profile(ctx._h, buf) == 0
        jobs.append(int(buf[16 * 8 + 4]))
        lds_jobs.append(int(buf[16 * 8 + 6]))
        twin_equal.append(bool(np.array_equal(out.rv(), res[resident]["rv"]) and np.array_equal(st.n_evals, res[resident]["evals"])))
        ctx.close()
    a, b = res[1], res[0]
    return dict(case=case, equal={k: bool(np.array_equal(a[k], b[k])) for k in ("rv", "epoch", "status", "acc", "rej", "evals")},
                ok=bool((a["status"] == 0).all() and (b["status"] == 0).all()), helpers=[a["helpers"], b["helpers"]], feed=[a["feed"], b["feed"]],
                jobs=jobs, lds_jobs=lds_jobs, twin_equal=twin_equal, evals=int(a["evals"].sum()), ms=[round(a["ms"], 2), round(b["ms"], 2)])


if __name__ == "__main__":
    print("RESULT " + json.dumps(run(sys.argv[1])), flush=True)
