"""CPU: the context builder (nyx_amd/csrc/ctx_build.h, used by nyx_hip_ctx_create in abi.cpp) as a stand-alone C++ check - g++ only,
no HIP, no GPU.  The BASELINE shapes of tests/cxx/launch_plan_cases.h and cases that reach every branch and every refusal of the
builder, each under three LDS sizes: every line equal to tests/golden/ctx_build.txt (written by the nyx_hip_ctx_create of the commit
before the builder moved out of abi.cpp, compiled on the host with HIP stubbed and the same LDS fakes)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ctx_build.txt")


def test_ctx_build_check(tmp_path):
    exe = str(tmp_path / "ctx_build_check")
    lines = str(tmp_path / "ctx_build.txt")
    subprocess.run(["g++", "-std=c++17", "-O2", os.path.join(ROOT, "tests", "cxx", "ctx_build_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe, lines], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert r.stdout.strip().endswith("ok")
    with open(lines) as f:
        got = f.read().splitlines()
    with open(GOLDEN) as f:
        want = f.read().splitlines()
    assert len(got) == len(want)
    diff = [(w, g) for w, g in zip(want, got) if w != g]
    assert not diff, f"{len(diff)} builds differ from the golden; first:\n  want {diff[0][0][:400]}\n  got  {diff[0][1][:400]}"


def test_the_builder_reads_no_environment():
    """The builder's inputs are its arguments: the environment route of the tuning stays in abi.cpp (resolve_tuning)."""
    src = open(os.path.join(ROOT, "nyx_amd", "csrc", "ctx_build.h")).read()
    assert "getenv" not in src and "environ" not in src
