"""CPU-side fence around the RIC kernels (ric_kernel.hip), the twin of tests/test_report_budget.py for the kernels with the
`nyxric_` prefix: VGPRs, scratch bytes per lane, static spill counts and .text bytes of every one of them
(tools/kernel_meta.py) are held to tests/golden/ric_budget.json - a figure above its budget fails with the number, a figure
more than 25 % BELOW its budget fails too (stale budget: `python tools/series_budget.py ric --update`), and the tests skip under
another hipcc than the one the budgets were written under.  On top of that the evaluation kernel, which runs the
interpolation of nyx_traj_eval_kernel TWICE per sample (run, then reference), may not use more scratch or spill more VGPRs
than that sibling's own budget (tests/golden/code_budget.json): the two interpolations are sequential so that their tables
are never live together.  No GPU needed."""
import json
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "nyx_amd", "libnyx_hip.so")
BUDGET = os.path.join(ROOT, "tests", "golden", "ric_budget.json")
SIBLING = os.path.join(ROOT, "tests", "golden", "code_budget.json")
KERNELS = {"init_kernel", "diff_kernel", "seal_kernel", "smooth_kernel", "moments_kernel"}

pytestmark = pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf") or shutil.which("objcopy") is None,
                                reason="no built library or no LLVM binutils here")

_CACHE = {}


def measured():
    import code_budget
    import series_budget
    want = json.load(open(BUDGET)).get("hipcc")
    have = code_budget.toolchain()
    if want and have and want != have:
        pytest.skip(f"budgets were written under hipcc {want}, this is {have}: python tools/series_budget.py ric --update")
    if "m" not in _CACHE:
        _CACHE["m"] = series_budget.measure(LIB, "ric")
    return _CACHE["m"]


def test_every_ric_kernel_is_inside_its_budget():
    budget = json.load(open(BUDGET))["kernels"]
    got = measured()
    assert set(budget) == KERNELS
    problems = []
    for kernel, b in budget.items():
        assert kernel in got, f"{kernel}: not in the library any more (python tools/series_budget.py ric --update)"
        for key, limit in b.items():
            v = got[kernel][key]
            if v > limit:
                problems.append(f"{kernel}.{key}: {v} > budget {limit}")
            elif key in ("scratch_bytes", "vgpr_spills", "text_bytes") and limit > 64 and v < 0.75 * limit:
                problems.append(f"{kernel}.{key}: {v} is more than 25 % under its budget {limit} - tighten it")
    new = sorted(set(got) - set(budget))
    assert not new, f"RIC kernels without a budget: {new}"
    assert not problems, "\n".join(problems)


def test_two_interpolations_per_sample_do_not_push_the_tables_into_scratch():
    sibling = json.load(open(SIBLING))["kernels"]["traj_eval_kernel"]
    got = measured()["diff_kernel"]
    assert got["scratch_bytes"] <= sibling["scratch_bytes"], (got, sibling)
    assert got["vgpr_spills"] <= sibling["vgpr_spills"], (got, sibling)
    # ... and there is ONE copy of HRMINT in it: the text stays near the sibling's, not twice it
    assert got["text_bytes"] < 1.5 * sibling["text_bytes"], (got, sibling)
    # the filter keeps its nine-sample windows of six components in registers
    assert measured()["smooth_kernel"]["scratch_bytes"] == 0 and measured()["smooth_kernel"]["vgpr_spills"] == 0


def test_ric_kernels_stay_out_of_the_other_fences():
    """tools/code_budget.py takes every kernel whose name contains `nyx_`, the report fence (tools/series_budget.py) every `nyxrep_` one: the
    RIC kernels carry another prefix."""
    import kernel_meta
    names = [k.get("name", "") for k in kernel_meta.kernels(LIB)]
    mine = [n for n in names if "nyxric_" in n]
    assert len(mine) == len(KERNELS) and not [n for n in mine if "nyx_" in n or "nyxrep_" in n], mine
