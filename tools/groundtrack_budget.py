#!/usr/bin/env python3
"""The code-object fence of the ground-track kernels (groundtrack_kernel.hip): what tests/test_groundtrack_budget.py measures on the built
library, and the tool that writes the committed budgets (tests/golden/groundtrack_budget.json):
`python tools/groundtrack_budget.py --update [slack]` = measured figures x (1 + slack, default 0.08), to be run - and its diff read -
when a change of those kernels is INTENDED to move them.  Same figures and rules as tools/code_budget.py; the ground-track kernels
carry a prefix of their own (`nyxgt_`) and a budget file of their own.  Folding the two files together is a follow-up."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import code_budget  # noqa: E402
import kernel_meta  # noqa: E402

PREFIX = "nyxgt_"
BUDGET = os.path.join(ROOT, "tests", "golden", "groundtrack_budget.json")


def measure(lib):
    out = {}
    for k in kernel_meta.kernels(lib):
        name = k.get("name", "")
        if PREFIX not in name:
            continue
        short = name.split(PREFIX)[1].split("kernel")[0].rstrip("_") + "_kernel"
        out[short] = {"vgprs": int(k.get("vgpr_count", 0)) + int(k.get("agpr_count", 0)), "scratch_bytes": int(k.get("private_segment_fixed_size", 0)),
                      "vgpr_spills": int(k.get("vgpr_spill_count", 0)), "sgpr_spills": int(k.get("sgpr_spill_count", 0)),
                      "text_bytes": int(k.get("text_bytes", 0))}
    return out


if __name__ == "__main__":
    m = measure(os.path.join(ROOT, "nyx_amd", "libnyx_hip.so"))
    if "--update" in sys.argv:
        i = sys.argv.index("--update")
        slack = float(sys.argv[i + 1]) if len(sys.argv) > i + 1 else 0.08
        up = lambda v: int(v * (1.0 + slack)) + (4 if v else 0)
        b = {"note": "budgets = the figures of the build they were written from x (1 + slack); see tests/test_groundtrack_budget.py", "slack": slack,
             "hipcc": code_budget.toolchain(), "kernels": {k: {f: (v if f == "vgprs" else up(v)) for f, v in d.items()} for k, d in m.items()}}
        with open(BUDGET, "w") as f:
            json.dump(b, f, indent=1, sort_keys=True)
            f.write("\n")
        print("wrote tests/golden/groundtrack_budget.json")
    else:
        print(json.dumps(m, indent=1, sort_keys=True))
