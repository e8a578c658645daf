#!/usr/bin/env python3
"""The code-object fence of the targeter kernels (target_kernel.hip, prefix `nyxtgt_`): what tests/test_target_budget.py measures on the built
library, and the tool that writes the committed budget: `python tools/target_budget.py --update [slack]` = measured figures
x (1 + slack, default 0.08), to be run - and its diff read - when a change of those kernels is INTENDED to move them.  The twin of
tools/lambert_budget.py: same figures and rules as tools/series_budget.py, whose five families stay as they are; this family is
measured through its `measure_prefix`."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import code_budget  # noqa: E402
import series_budget  # noqa: E402

PREFIX, BUDGET = "nyxtgt_", "target_budget.json"


def measure(lib):
    return series_budget.measure_prefix(lib, PREFIX)


if __name__ == "__main__":
    m = measure(os.path.join(ROOT, "nyx_amd", "libnyx_hip.so"))
    if "--update" in sys.argv:
        i = sys.argv.index("--update")
        slack = float(sys.argv[i + 1]) if len(sys.argv) > i + 1 else 0.08
        up = lambda v: int(v * (1.0 + slack)) + (4 if v else 0)
        b = {"note": "budgets = the figures of the build they were written from x (1 + slack); see tests/test_target_budget.py", "slack": slack,
             "hipcc": code_budget.toolchain(), "kernels": {k: {f: (v if f == "vgprs" else up(v)) for f, v in d.items()} for k, d in m.items()}}
        with open(os.path.join(ROOT, "tests", "golden", BUDGET), "w") as f:
            json.dump(b, f, indent=1, sort_keys=True)
            f.write("\n")
        print(f"wrote tests/golden/{BUDGET}")
    else:
        print(json.dumps(m, indent=1, sort_keys=True))
