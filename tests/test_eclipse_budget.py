"""CPU-side fence around the eclipse kernels (eclipse_kernel.hip), the twin of tests/test_aer_budget.py for the kernels with the
`nyxecl_` prefix: VGPRs, scratch bytes per lane, static spill counts and .text bytes of every one of them (tools/kernel_meta.py)
are held to tests/golden/eclipse_budget.json - a figure above its budget fails with the number, a figure more than 25 % BELOW its
budget fails too (stale budget: `python tools/series_budget.py ecl --update`), and the tests skip under another hipcc than the one
the budgets were written under.  On top of that the evaluation kernel, which runs the interpolation of nyx_traj_eval_kernel in
its first pass and the ephemerides, the disk overlap and the parameters in its second, may not use more scratch or spill more
VGPRs than that sibling's own budget (tests/golden/code_budget.json): the second pass must not push HRMINT's tables out of
registers.  Register and scratch figures are read from the code object's metadata only.  No GPU needed."""
import json
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
LIB = os.path.join(ROOT, "nyx_amd", "libnyx_hip.so")
BUDGET = os.path.join(ROOT, "tests", "golden", "eclipse_budget.json")
SIBLING = os.path.join(ROOT, "tests", "golden", "code_budget.json")

pytestmark = pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf") or shutil.which("objcopy") is None,
                                reason="no built library or no LLVM binutils here")

_CACHE = {}


def measured():
    import code_budget
    import series_budget
    want = json.load(open(BUDGET)).get("hipcc")
    have = code_budget.toolchain()
    if want and have and want != have:
        pytest.skip(f"budgets were written under hipcc {want}, this is {have}: python tools/series_budget.py ecl --update")
    if "m" not in _CACHE:
        _CACHE["m"] = series_budget.measure(LIB, "ecl")
    return _CACHE["m"]


def test_every_eclipse_kernel_is_inside_its_budget():
    budget = json.load(open(BUDGET))["kernels"]
    got = measured()
    assert set(budget) == {"init_kernel", "values_kernel", "seal_kernel"}
    problems = []
    for kernel, b in budget.items():
        assert kernel in got, f"{kernel}: not in the library any more (python tools/series_budget.py ecl --update)"
        for key, limit in b.items():
            v = got[kernel][key]
            if v > limit:
                problems.append(f"{kernel}.{key}: {v} > budget {limit}")
            elif key in ("scratch_bytes", "vgpr_spills", "text_bytes") and limit > 64 and v < 0.75 * limit:
                problems.append(f"{kernel}.{key}: {v} is more than 25 % under its budget {limit} - tighten it")
    new = sorted(set(got) - set(budget))
    assert not new, f"eclipse kernels without a budget: {new}"
    assert not problems, "\n".join(problems)


def test_the_second_pass_does_not_push_the_interpolation_into_scratch():
    sibling = json.load(open(SIBLING))["kernels"]["traj_eval_kernel"]
    got = measured()["values_kernel"]
    assert got["scratch_bytes"] <= sibling["scratch_bytes"], (got, sibling)
    assert got["vgpr_spills"] <= sibling["vgpr_spills"], (got, sibling)


def test_eclipse_kernels_stay_out_of_the_other_fences():
    """tools/code_budget.py takes every kernel whose name contains `nyx_`, the report, RIC, ground-track and station-view fences
    `nyxrep_` / `nyxric_` / `nyxgt_` / `nyxaer_`: the eclipse kernels carry another prefix, and there are exactly three of them."""
    import kernel_meta
    import series_budget
    names = [k.get("name", "") for k in kernel_meta.kernels(LIB)]
    mine = [n for n in names if "nyxecl_" in n]
    assert len(mine) == 3 and not [n for n in mine if "nyx_" in n or "nyxrep_" in n or "nyxric_" in n or "nyxgt_" in n or "nyxaer_" in n], mine
    assert sorted(n.split("nyxecl_")[1].split("kernel")[0] for n in mine) == ["init_", "seal_", "values_"]
    assert series_budget.FAMILIES["ecl"] == ("nyxecl_", "eclipse_budget.json")
    for family, (prefix, _) in series_budget.FAMILIES.items():
        if family != "ecl":
            assert not [n for n in names if prefix in n and "nyxecl_" in n], family
