"""CPU: the code of the station-view kernels holds no register copy under a one-sided exec mask (tools/flow_copy_check.py).

The first shape of csrc/aer_kernel.hip - the station loop inside the sample loop - was MISCOMPILED: the register allocator parked the
first epoch of the lane's series in AGPRs with two `v_accvgpr_write_b32` placed in the structurizer's Flow block of a divergent
branch every lane leaves by the other side, so they ran with an empty exec mask and the reload returned stale registers; on the
MI355X every series ended at its third sample (profiles/HISTORY.md, "Station views").  Nothing in the code-object metadata shows
that.  This test compiles the translation unit (gfx950, the flags of the build, a few seconds) and walks its assembly: the checker
must find the pattern in a hand-written snippet, and none in the kernel.  Skipped without hipcc."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

SNIPPET = """
_Z6kernelv:
.LBB0_1:
	s_and_saveexec_b64 s[6:7], vcc
	s_xor_b64 s[6:7], exec, s[6:7]
	s_cbranch_execz .LBB0_3
; %bb.2:
	v_accvgpr_write_b32 a9, v1
.LBB0_3:                                ; %Flow1240
	v_accvgpr_write_b32 a4, v46
	v_writelane_b32 v255, s6, 31
	s_andn2_saveexec_b64 s[6:7], s[6:7]
	v_accvgpr_write_b32 a5, v47
.LBB0_4:                                ; %Flow12
	s_or_b64 exec, exec, s[6:7]
	v_accvgpr_write_b32 a6, v48
"""


def test_the_checker_finds_a_copy_between_a_flow_label_and_the_next_write_of_exec():
    import flow_copy_check
    assert flow_copy_check.flow_copies(SNIPPET) == [("_Z6kernelv", 10, "v_accvgpr_write_b32 a4, v46")]
    # the flags the checker compiles with are the ones the build compiles with
    build = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "flags = [" + ", ".join(f'"{f}"' for f in flow_copy_check.FLAGS) + "]" in build


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="no hipcc here")
def test_the_station_view_kernels_hold_no_copy_under_a_one_sided_exec_mask():
    import flow_copy_check
    asm = flow_copy_check.assembly(os.path.join(ROOT, "nyx_amd", "csrc", "aer_kernel.hip"))
    assert "nyxaer_values_kernel" in asm and asm.count("%Flow") > 10       # (the labels the checker reads are there)
    assert flow_copy_check.flow_copies(asm) == []
