"""CPU-side fence around the link kernels (`nyxlnk_`, link_kernel.hip), the twin of tests/test_frame_budget.py for the family of
tools/link_budget.py: VGPRs, scratch bytes per lane, static spill counts and .text bytes of the three kernels
(tools/kernel_meta.py) are held to tests/golden/link_budget.json - a figure above its budget fails with the number, a figure more
than 25 % BELOW its budget fails too (stale budget: `python tools/link_budget.py --update`), and the tests skip under another hipcc
than the one the budget was written under.  On top of that the evaluation kernel, which runs the interpolation of
nyx_traj_eval_kernel twice per sample (one rolled loop, one copy) plus its own second pass (the ephemerides, the SIGHT test, the
parameters), may not use more scratch or spill more VGPRs than that sibling's own budget (tests/golden/code_budget.json): what is
added must not push HRMINT's tables out of registers.  Register and scratch figures are read from the code object's metadata only.
No GPU needed."""
import json
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import frame_budget  # noqa: E402
import link_budget  # noqa: E402
import series_budget  # noqa: E402

LIB = os.path.join(ROOT, "nyx_amd", "libnyx_hip.so")
SIBLING = os.path.join(ROOT, "tests", "golden", "code_budget.json")
THREE = {"init_kernel", "values_kernel", "seal_kernel"}

pytestmark = pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf") or shutil.which("objcopy") is None,
                                reason="no built library or no LLVM binutils here")

_CACHE = {}


def code_budget_names():
    return json.load(open(SIBLING))["kernels"]


def budget():
    return json.load(open(os.path.join(ROOT, "tests", "golden", link_budget.BUDGET)))


def measured():
    import code_budget
    want = budget().get("hipcc")
    have = code_budget.toolchain()
    if want and have and want != have:
        pytest.skip(f"the budget was written under hipcc {want}, this is {have}: python tools/link_budget.py --update")
    if "m" not in _CACHE:
        _CACHE["m"] = link_budget.measure(LIB)
    return _CACHE["m"]


def test_every_kernel_is_inside_its_budget():
    kernels = budget()["kernels"]
    got = measured()
    assert set(kernels) == THREE
    problems = []
    for kernel, b in kernels.items():
        assert kernel in got, f"{kernel}: not in the library any more (python tools/link_budget.py --update)"
        for key, limit in b.items():
            v = got[kernel][key]
            if v > limit:
                problems.append(f"{kernel}.{key}: {v} > budget {limit}")
            elif key in ("scratch_bytes", "vgpr_spills", "text_bytes") and limit > 64 and v < 0.75 * limit:
                problems.append(f"{kernel}.{key}: {v} is more than 25 % under its budget {limit} - tighten it")
    new = sorted(set(got) - set(kernels))
    assert not new, f"link kernels without a budget: {new}"
    assert not problems, "\n".join(problems)


def test_the_evaluation_kernel_does_not_push_the_interpolation_into_scratch():
    """(and the one rolled loop around `traj_at` keeps ONE copy of the interpolation: the text is not twice a sibling's)"""
    sibling = json.load(open(SIBLING))["kernels"]["traj_eval_kernel"]
    got = measured()["values_kernel"]
    assert got["scratch_bytes"] <= sibling["scratch_bytes"], (got, sibling)
    assert got["vgpr_spills"] <= sibling["vgpr_spills"], (got, sibling)


def test_the_kernels_stay_out_of_the_other_fences():
    """tools/code_budget.py takes every kernel whose name contains `nyx_`, every family of tools/series_budget.py those with its prefix,
    tools/frame_budget.py those with `nyxfrm_`: the link kernels carry `nyxlnk_` and none of those, they are exactly the three
    budgeted, and the five families and the encounter fence are as they were."""
    import kernel_meta
    assert sorted(series_budget.FAMILIES) == ["aer", "ecl", "groundtrack", "report", "ric"] and link_budget.PREFIX == "nyxlnk_"
    others = ["nyx_", frame_budget.PREFIX] + [p for p, _ in series_budget.FAMILIES.values()]
    assert not [o for o in others if o in link_budget.PREFIX or link_budget.PREFIX in o]
    names = [k.get("name", "") for k in kernel_meta.kernels(LIB)]
    mine = [n for n in names if link_budget.PREFIX in n]
    assert len(mine) == 3 and not [n for n in mine if any(o in n for o in others)], mine
    assert {n.split(link_budget.PREFIX)[1].split("kernel")[0] + "kernel" for n in mine} == THREE
    assert set(frame_budget.measure(LIB)) == THREE and not [k for k in code_budget_names() if "lnk" in k]
    for family in series_budget.FAMILIES:                      # and no family's measure picks them up
        assert not [k for k in series_budget.measure(LIB, family) if k not in json.load(open(os.path.join(ROOT, "tests", "golden", series_budget.FAMILIES[family][1])))["kernels"]]
