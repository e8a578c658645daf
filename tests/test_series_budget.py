"""CPU-side fences around the kernels of the five fused trajectory reports, the twins of tests/test_code_budget.py for the families
of tools/series_budget.py - report (`nyxrep_`, report_kernel.hip), ric (`nyxric_`, ric_kernel.hip), groundtrack (`nyxgt_`,
groundtrack_kernel.hip), aer (`nyxaer_`, aer_kernel.hip) and ecl (`nyxecl_`, eclipse_kernel.hip): VGPRs, scratch bytes per lane, static
spill counts and .text bytes of every kernel (tools/kernel_meta.py) are held to the family's tests/golden/*_budget.json - a figure
above its budget fails with the number, a figure more than 25 % BELOW its budget fails too (stale budget: `python
tools/series_budget.py FAMILY --update`), and the tests skip under another hipcc than the one the budgets were written under.  On top
of that the evaluation kernel of a family, which runs the interpolation of nyx_traj_eval_kernel plus its own block (the parameters;
the frame; the stations; the ephemerides and the disk overlap in a second pass; for RIC a second, sequential interpolation), may not
use more scratch or spill more VGPRs than that sibling's own budget (tests/golden/code_budget.json): what is added must not push
HRMINT's tables out of registers.  Register and scratch figures are read from the code object's metadata only.  No GPU needed."""
import json
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import series_budget  # noqa: E402

LIB = os.path.join(ROOT, "nyx_amd", "libnyx_hip.so")
SIBLING = os.path.join(ROOT, "tests", "golden", "code_budget.json")
# family -> ((prefix, budget file) as tools/series_budget.py must hold it, its kernels, its evaluation kernel)
THREE = {"init_kernel", "values_kernel", "seal_kernel"}
PINNED = {"report": (("nyxrep_", "report_budget.json"), THREE, "values_kernel"),
          "ric": (("nyxric_", "ric_budget.json"), {"init_kernel", "diff_kernel", "seal_kernel", "smooth_kernel", "moments_kernel"}, "diff_kernel"),
          "groundtrack": (("nyxgt_", "groundtrack_budget.json"), THREE, "values_kernel"),
          "aer": (("nyxaer_", "aer_budget.json"), THREE, "values_kernel"),
          "ecl": (("nyxecl_", "eclipse_budget.json"), THREE, "values_kernel")}

NEEDS = pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf") or shutil.which("objcopy") is None,
                           reason="no built library or no LLVM binutils here")
pytestmark = [NEEDS, pytest.mark.parametrize("family", sorted(series_budget.FAMILIES))]

_CACHE = {}


def budget_of(family):
    return json.load(open(os.path.join(ROOT, "tests", "golden", PINNED[family][0][1])))


def measured(family):
    import code_budget
    want = budget_of(family).get("hipcc")
    have = code_budget.toolchain()
    if want and have and want != have:
        pytest.skip(f"budgets were written under hipcc {want}, this is {have}: python tools/series_budget.py {family} --update")
    if family not in _CACHE:
        _CACHE[family] = series_budget.measure(LIB, family)
    return _CACHE[family]


def test_every_kernel_is_inside_its_budget(family):
    budget = budget_of(family)["kernels"]
    got = measured(family)
    assert set(budget) == PINNED[family][1]
    problems = []
    for kernel, b in budget.items():
        assert kernel in got, f"{kernel}: not in the library any more (python tools/series_budget.py {family} --update)"
        for key, limit in b.items():
            v = got[kernel][key]
            if v > limit:
                problems.append(f"{kernel}.{key}: {v} > budget {limit}")
            elif key in ("scratch_bytes", "vgpr_spills", "text_bytes") and limit > 64 and v < 0.75 * limit:
                problems.append(f"{kernel}.{key}: {v} is more than 25 % under its budget {limit} - tighten it")
    new = sorted(set(got) - set(budget))
    assert not new, f"{family} kernels without a budget: {new}"
    assert not problems, "\n".join(problems)


def test_the_evaluation_kernel_does_not_push_the_interpolation_into_scratch(family):
    sibling = json.load(open(SIBLING))["kernels"]["traj_eval_kernel"]
    got = measured(family)[PINNED[family][2]]
    assert got["scratch_bytes"] <= sibling["scratch_bytes"], (got, sibling)
    assert got["vgpr_spills"] <= sibling["vgpr_spills"], (got, sibling)
    if family == "ric":
        # ... and there is ONE copy of HRMINT in it (the two interpolations are sequential): the text stays near the sibling's, not twice it
        assert got["text_bytes"] < 1.5 * sibling["text_bytes"], (got, sibling)
        # the filter keeps its nine-sample windows of six components in registers
        assert measured(family)["smooth_kernel"]["scratch_bytes"] == 0 and measured(family)["smooth_kernel"]["vgpr_spills"] == 0


def test_the_kernels_stay_out_of_the_other_fences(family):
    """tools/code_budget.py takes every kernel whose name contains `nyx_`, every family here those with its prefix: the kernels of a
    family carry that prefix and no other, and they are exactly the ones budgeted."""
    import kernel_meta
    assert set(series_budget.FAMILIES) == set(PINNED) and series_budget.FAMILIES[family] == PINNED[family][0]
    (prefix, _), kernels, _ = PINNED[family]
    others = ["nyx_"] + [p for f, ((p, _), _, _) in PINNED.items() if f != family]
    names = [k.get("name", "") for k in kernel_meta.kernels(LIB)]
    mine = [n for n in names if prefix in n]
    assert len(mine) == len(kernels) and not [n for n in mine if any(o in n for o in others)], mine
    assert {n.split(prefix)[1].split("kernel")[0] + "kernel" for n in mine} == kernels
