#!/usr/bin/env python3
"""The code-object fences of the five fused trajectory reports - the report kernels (report_kernel.hip), the RIC kernels
(ric_kernel.hip), the ground-track kernels (groundtrack_kernel.hip), the station-view kernels (aer_kernel.hip) and the eclipse
kernels (eclipse_kernel.hip): what tests/test_series_budget.py measures on the built library, and the tool that writes the committed budgets:
`python tools/series_budget.py FAMILY --update [slack]` (FAMILY = report, ric, groundtrack, aer or ecl) = measured figures x (1 + slack,
default 0.08), to be run - and its diff read - when a change of those kernels is INTENDED to move them.  Same figures and rules as
tools/code_budget.py; each family carries a kernel-name prefix and a budget file of its own."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import code_budget  # noqa: E402
import kernel_meta  # noqa: E402

FAMILIES = {"report": ("nyxrep_", "report_budget.json"), "ric": ("nyxric_", "ric_budget.json"), "groundtrack": ("nyxgt_", "groundtrack_budget.json"),
            "aer": ("nyxaer_", "aer_budget.json"), "ecl": ("nyxecl_", "eclipse_budget.json")}


def measure(lib, family):
    return measure_prefix(lib, FAMILIES[family][0])


def measure_prefix(lib, prefix):
    """The figures of every kernel of `lib` whose name holds `prefix` (a family of FAMILIES, or one with a tool of its own:
    tools/frame_budget.py)."""
    out = {}
    for k in kernel_meta.kernels(lib):
        name = k.get("name", "")
        if prefix not in name:
            continue
        short = name.split(prefix)[1].split("kernel")[0].rstrip("_") + "_kernel"
        out[short] = {"vgprs": int(k.get("vgpr_count", 0)) + int(k.get("agpr_count", 0)), "scratch_bytes": int(k.get("private_segment_fixed_size", 0)),
                      "vgpr_spills": int(k.get("vgpr_spill_count", 0)), "sgpr_spills": int(k.get("sgpr_spill_count", 0)),
                      "text_bytes": int(k.get("text_bytes", 0))}
    return out


if __name__ == "__main__":
    if len(sys.argv) < 2 or sys.argv[1] not in FAMILIES:
        sys.exit(f"usage: series_budget.py {{{' | '.join(FAMILIES)}}} [--update [slack]]")
    family = sys.argv[1]
    m = measure(os.path.join(ROOT, "nyx_amd", "libnyx_hip.so"), family)
    if "--update" in sys.argv:
        i = sys.argv.index("--update")
        slack = float(sys.argv[i + 1]) if len(sys.argv) > i + 1 else 0.08
        up = lambda v: int(v * (1.0 + slack)) + (4 if v else 0)
        b = {"note": f"budgets = the figures of the build they were written from x (1 + slack); see tests/test_{FAMILIES[family][1][:-5]}.py", "slack": slack,
             "hipcc": code_budget.toolchain(), "kernels": {k: {f: (v if f == "vgprs" else up(v)) for f, v in d.items()} for k, d in m.items()}}
        with open(os.path.join(ROOT, "tests", "golden", FAMILIES[family][1]), "w") as f:
            json.dump(b, f, indent=1, sort_keys=True)
            f.write("\n")
        print(f"wrote tests/golden/{FAMILIES[family][1]}")
    else:
        print(json.dumps(m, indent=1, sort_keys=True))
