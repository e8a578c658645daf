"""CPU: the code of the link kernels holds no register copy under a one-sided exec mask (tools/flow_copy_check.py), the twin of
tests/test_frame_flow_copies.py.

The link evaluation kernel has the two-pass tile shape of csrc/aer_kernel.hip and csrc/eclipse_kernel.hip because the shape with the
value block inside the sample loop was MISCOMPILED for the station views: copies to AGPRs placed in the structurizer's Flow block of
a divergent branch ran with an empty exec mask (profiles/HISTORY.md, "Station views").  This kernel runs the interpolation twice per
sample in a rolled loop inside its first pass and does use AGPRs, so the existing checker is applied to its translation unit as
well: compiled for gfx950 with the flags of the build (a few seconds), its assembly must hold no such copy.  Nothing in the
code-object metadata would show one.  Skipped without hipcc."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="no hipcc here")
def test_the_link_kernels_hold_no_copy_under_a_one_sided_exec_mask():
    import flow_copy_check
    asm = flow_copy_check.assembly(os.path.join(ROOT, "nyx_amd", "csrc", "link_kernel.hip"))
    assert "nyxlnk_values_kernel" in asm and asm.count("%Flow") > 10       # (the labels the checker reads are there)
    assert flow_copy_check.flow_copies(asm) == []
    # the LDS columns reach csrc/link_dev.h as plain pointers: after inlining they are LDS accesses again, not flat ones
    assert "flat_load" not in asm and "flat_store" not in asm and "ds_read" in asm and "ds_write" in asm
