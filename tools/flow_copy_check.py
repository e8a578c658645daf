#!/usr/bin/env python3
"""Looks for register copies that the compiler placed where the exec mask is that of ONE side of a divergent branch.

The register allocator of hipcc splits long live ranges with copies (VGPR -> AGPR `v_accvgpr_write_b32`, or stores to scratch) at the
boundary of a high-pressure region.  When that boundary is the structurizer's "Flow" block of a divergent branch - reached through
`s_cbranch_execz`, before `s_or_b64 exec` / `s_andn2_saveexec_b64` rejoin the mask - the copy runs for the lanes of one side only,
with NO lane when every lane took the other side, and the reload behind the region, under the full mask, returns stale registers.
The first shape of csrc/aer_kernel.hip was miscompiled that way (profiles/HISTORY.md, "Station views").

This tool compiles one translation unit for gfx950 with the flags of the build and `-save-temps`, walks the assembly and prints every
such copy: an instruction of COPIES in a block whose label carries `%Flow`, before the first instruction of that block that writes
exec.  `v_writelane_b32` (SGPR spills) is not masked by exec and is not reported.  Exit status 1 when anything was found.
usage: python tools/flow_copy_check.py nyx_amd/csrc/aer_kernel.hip [more.hip ...]"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wno-unused-value"]   # those of __graft_entry__.build
COPIES = ("v_accvgpr_write", "scratch_store", "buffer_store")
EXEC_WRITE = re.compile(r"s_\w+_b64\s+exec\b|s_\w*saveexec_b64")


def assembly(source):
    """The gfx950 assembly of one translation unit, as text."""
    with tempfile.TemporaryDirectory() as td:
        subprocess.run(["hipcc", *FLAGS, "-save-temps=obj", "-c", os.path.abspath(source), "-o", os.path.join(td, "tu.o")], check=True, cwd=td,
                       capture_output=True)
        name = [f for f in os.listdir(td) if f.endswith(".s") and "amdgcn" in f]
        assert len(name) == 1, name
        return open(os.path.join(td, name[0])).read()


def flow_copies(asm):
    """[(function, line number, instruction)] of the copies found in `asm`."""
    found, function, in_flow = [], None, False
    for no, line in enumerate(asm.splitlines(), 1):
        m = re.match(r"^(\w+):", line)
        if m and not line.startswith(".L"):
            function, in_flow = m.group(1), False
        if re.match(r"^\.LBB\d+_\d+:", line):
            in_flow = "%Flow" in line
            continue
        text = line.strip()
        if not in_flow or not text or text.startswith(";"):
            continue
        if EXEC_WRITE.match(text):
            in_flow = False
        elif text.startswith(COPIES):
            found.append((function, no, text))
    return found


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    bad = 0
    for src in sys.argv[1:]:
        hits = flow_copies(assembly(src))
        for function, no, text in hits:
            print(f"{src}: {function}: line {no}: {text}")
        print(f"{src}: {len(hits)} copies under a one-sided exec mask")
        bad += len(hits)
    sys.exit(1 if bad else 0)
