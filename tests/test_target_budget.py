"""CPU-side fence around the targeter kernels (`nyxtgt_`, target_kernel.hip), after tests/test_lambert_budget.py for the family of
tools/target_budget.py: VGPRs, scratch bytes per lane, static spill counts and .text bytes of the two kernels (tools/kernel_meta.py)
are held to tests/golden/target_budget.json - a figure above its budget fails with the number, a figure more than 25 % BELOW its budget
fails too (stale budget: `python tools/target_budget.py --update`), and the tests skip under another hipcc than the one the budget was
written under.  On top of that both kernels stay out of scratch and spill no vector register, and the step kernel keeps at least two
waves a SIMD (at most 256 VGPRs): its VGPR count is recorded, not gated beyond that.  What the metadata counts as SGPR spills are
scalars parked in the lanes of a VECTOR REGISTER (the kernels' argument block is larger than the scalar file): no memory is involved;
they are recorded in the budget like the other figures.  Register and scratch figures are read from the code object's metadata only.
No GPU needed."""
import json
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import frame_budget  # noqa: E402
import lambert_budget  # noqa: E402
import link_budget  # noqa: E402
import series_budget  # noqa: E402
import stats_budget  # noqa: E402
import target_budget  # noqa: E402

LIB = os.path.join(ROOT, "nyx_amd", "libnyx_hip.so")
TWO = {"seed_kernel", "step_kernel"}

pytestmark = pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf") or shutil.which("objcopy") is None,
                                reason="no built library or no LLVM binutils here")

_CACHE = {}


def budget():
    return json.load(open(os.path.join(ROOT, "tests", "golden", target_budget.BUDGET)))


def measured():
    import code_budget
    want = budget().get("hipcc")
    have = code_budget.toolchain()
    if want and have and want != have:
        pytest.skip(f"the budget was written under hipcc {want}, this is {have}: python tools/target_budget.py --update")
    if "m" not in _CACHE:
        _CACHE["m"] = target_budget.measure(LIB)
    return _CACHE["m"]


def test_every_kernel_is_inside_its_budget():
    kernels = budget()["kernels"]
    got = measured()
    assert set(kernels) == TWO
    problems = []
    for kernel, b in kernels.items():
        assert kernel in got, f"{kernel}: not in the library any more (python tools/target_budget.py --update)"
        for key, limit in b.items():
            v = got[kernel][key]
            if v > limit:
                problems.append(f"{kernel}.{key}: {v} > budget {limit}")
            elif key in ("scratch_bytes", "vgpr_spills", "text_bytes") and limit > 64 and v < 0.75 * limit:
                problems.append(f"{kernel}.{key}: {v} is more than 25 % under its budget {limit} - tighten it")
    new = sorted(set(got) - set(kernels))
    assert not new, f"targeter kernels without a budget: {new}"
    assert not problems, "\n".join(problems)


def test_no_scratch_no_vector_spills_and_two_waves_a_simd():
    got = measured()
    for kernel, g in got.items():
        assert g["scratch_bytes"] == 0 and g["vgpr_spills"] == 0, (kernel, g)
    print("VGPRs:", {k: g["vgprs"] for k, g in got.items()})
    assert got["step_kernel"]["vgprs"] <= 256, got["step_kernel"]     # 512 registers a lane of a SIMD: two waves


def test_the_kernels_stay_out_of_the_other_fences():
    """tools/code_budget.py takes every kernel whose name contains `nyx_`, every other family those with its prefix: the targeter
    kernels carry `nyxtgt_` and none of those, they are exactly the two budgeted, and no other measure picks them up."""
    import kernel_meta
    assert target_budget.PREFIX == "nyxtgt_"
    others = ["nyx_", frame_budget.PREFIX, link_budget.PREFIX, stats_budget.PREFIX, lambert_budget.PREFIX] + [p for p, _ in series_budget.FAMILIES.values()]
    assert not [o for o in others if o in target_budget.PREFIX or target_budget.PREFIX in o]
    names = [k.get("name", "") for k in kernel_meta.kernels(LIB)]
    mine = [n for n in names if target_budget.PREFIX in n]
    assert len(mine) == 2 and not [n for n in mine if any(o in n for o in others)], mine
    assert {n.split(target_budget.PREFIX)[1].split("kernel")[0] + "kernel" for n in mine} == TWO
    code = json.load(open(os.path.join(ROOT, "tests", "golden", "code_budget.json")))["kernels"]
    assert not [k for k in code if "tgt" in k]
    for tool in (frame_budget, link_budget, stats_budget, lambert_budget):
        assert not set(tool.measure(LIB)) & TWO
