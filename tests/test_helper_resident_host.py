"""CPU: the host side of the helpers' resident feed as a stand-alone C++ check (tests/cxx/helper_resident_check.cpp) - g++ only, no
HIP, no GPU.  The block a helper workgroup stages in LDS is the vector side of the helpers' run stream: the rows of its schedule's
columns, every range at the head of a sixteen-row group, sized by `run_stream_groups`; and the selection follows the fit rule
(`select_helper_feed`: claim mode, one-part hand-off, sixteen waves, a block of at most 80 KB, `tuning.helper_resident` not 0)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_helper_resident_check(tmp_path):
    exe = str(tmp_path / "helper_resident_check")
    subprocess.run(["g++", "-std=c++17", "-O2", os.path.join(ROOT, "tests", "cxx", "helper_resident_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert r.stdout.strip().endswith("ok")
    assert "headline (70x70, 10 000 trajectories)" in r.stdout and "not staged" in r.stdout


def test_resident_loop_header_is_up_to_date():
    """The committed harm_resident_asm.h is, byte for byte, what tools/gen_harm_stream.py emits (importing the generator writes the
    streamed header only; this one is written when the generator is run)."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_harm_stream as g
    committed = open(os.path.join(ROOT, "nyx_amd", "csrc", "harm_resident_asm.h")).read()
    text, count = g.header(True)
    assert committed == text and count > 900
    assert g.header(False)[0] == open(g.OUT).read()


def test_the_resident_loop_is_the_streamed_loop_with_other_group_loads():
    """Both generated loops come from one generator: row for row the same instructions, and the resident one touches no global memory."""
    def rows(path):
        text = open(os.path.join(ROOT, "nyx_amd", "csrc", path)).read()
        return [ln.strip() for ln in text.splitlines() if '"v_' in ln and "v_add_u32" not in ln], text
    stream, stream_text = rows("harm_stream_asm.h")
    resident, resident_text = rows("harm_resident_asm.h")
    assert stream == resident and len(stream) > 32 * 9
    assert "global_load" not in resident_text and "vmcnt" not in resident_text
    assert resident_text.count("ds_read_b64") == stream_text.count("global_load_dwordx2") == 16
    # every group load of the resident loop is retired by the batch load's wait behind it, before any row (the generator's wait rule)
    lines = re.findall(r'^\s+"(.*?)\\n\\t" \\$', resident_text, flags=re.M)  # the instructions and labels of the asm statement
    for k, ln in enumerate(lines):
        if ln.startswith("ds_read_b64"):
            rest = lines[k + 1:]
            wait = next(i for i, x in enumerate(rest) if x.startswith("s_waitcnt lgkmcnt(0)"))
            dpp = next((i for i, x in enumerate(rest) if "_dpp" in x), len(rest))  # (the last group: behind it the loop branches to its top)
            assert wait < dpp, ln
    top = lines.index(".Lhs_top_%=:")
    assert [x for x in lines[top + 1:top + 6] if x.startswith("s_waitcnt")] == ["s_waitcnt lgkmcnt(0)"]
