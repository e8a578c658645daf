"""CPU: the memory of a context (nyx_amd/csrc/ctx_mem.h, used by abi.cpp) and build_run_stream (nyx_amd/csrc/ctx_build.h) as a
stand-alone C++ check - g++ only, no HIP, no GPU.  The blocks of a batch's arrays (with and without the stats rows), of the
cooperative-mode mailboxes and of what the targeter keeps against the expressions abi.cpp carried inline before the header had them,
at capacities 1 .. 1 000 000; the owner and its one grow rule on a counting allocator (no call at or below the capacity, quiesce
once and before the free, never on an empty owner, empty after a failed allocation, move, every allocation freed exactly once);
build_run_stream against the function as abi.cpp carried it, on the schedules of a 2x0, an 8x8 and the JGM3 70x70 field.  The same
program once more under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cxx", "ctx_mem_check.cpp")
JGM3 = os.path.join(ROOT, "nyx_amd", "data", "jgm3_70x70.f64")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_ctx_mem_check(tmp_path, flags):
    exe = str(tmp_path / "ctx_mem_check")
    subprocess.run(["g++", "-std=c++17", *flags, SRC, "-o", exe], check=True)
    r = subprocess.run([exe, JGM3], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.strip().endswith("ok")


def test_the_ctx_mem_header_reads_no_environment():
    """Host only: no environment, no HIP runtime."""
    src = open(os.path.join(ROOT, "nyx_amd", "csrc", "ctx_mem.h")).read()
    assert "getenv" not in src and "environ" not in src and "hip_runtime" not in src
