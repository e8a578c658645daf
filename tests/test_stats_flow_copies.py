"""CPU: the code of the statistics kernels holds no register copy under a one-sided exec mask (tools/flow_copy_check.py), the twin of
tests/test_link_flow_copies.py.

The checker exists because a kernel of the station views was MISCOMPILED: copies placed in the structurizer's Flow block of a
divergent branch ran with an empty exec mask (profiles/HISTORY.md, "Station views").  The statistics kernel has divergent branches of
its own - a slot that is not held, a key outside the prefix of a radix pass, the one thread that finds the bin - around LDS atomics,
so the existing checker is applied to its translation unit as well: compiled for gfx950 with the flags of the build (a few seconds),
its assembly must hold no such copy.  Nothing in the code-object metadata would show one.  Skipped without hipcc."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="no hipcc here")
def test_the_statistics_kernels_hold_no_copy_under_a_one_sided_exec_mask():
    import flow_copy_check
    asm = flow_copy_check.assembly(os.path.join(ROOT, "nyx_amd", "csrc", "stats_kernel.hip"))
    assert "nyxstat_lds_kernel" in asm and "nyxstat_global_kernel" in asm and asm.count("%Flow") > 10    # (the labels the checker reads are there)
    assert flow_copy_check.flow_copies(asm) == []
    # the keys are LDS accesses, the histogram LDS atomics of integers; no floating-point atomic anywhere
    assert "ds_read" in asm and "ds_write" in asm and "ds_add_u32" in asm and "ds_min_u64" in asm
    assert "atomic_add_f" not in asm and "ds_add_f" not in asm
