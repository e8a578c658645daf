"""CPU: the launch planner (nyx_amd/csrc/launch_plan.h, used by launch() in abi.cpp) as a stand-alone C++ check - g++ only, no HIP,
no GPU.  The BASELINE workloads' shapes (tests/cxx/launch_plan_cases.h) at eight ensemble sizes under the tuning variants the GPU tests
use: every plan at 256 CUs equal to tests/golden/launch_plans.txt.gz (written by the launch() of the commit before the planner moved
out of abi.cpp), every column dealt exactly once, the mailbox block large enough, the helper counts the GPU tests expect of a 256-CU
device, and no cooperative build failing at default tuning for degrees 8..150."""
import gzip
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_plans.txt.gz")


def test_launch_plan_check(tmp_path):
    exe = str(tmp_path / "launch_plan_check")
    plans = str(tmp_path / "plans.txt")
    subprocess.run(["g++", "-std=c++17", "-O2", os.path.join(ROOT, "tests", "cxx", "launch_plan_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe, plans], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert r.stdout.strip().endswith("ok")
    assert "none fails" in r.stdout and "264 answer blocks" in r.stdout
    with open(plans) as f:
        got = f.read().splitlines()
    with gzip.open(GOLDEN, "rt") as f:
        want = f.read().splitlines()
    assert len(got) == len(want)
    diff = [(w, g) for w, g in zip(want, got) if w != g]
    assert not diff, f"{len(diff)} plans differ from the golden; first:\n  want {diff[0][0][:400]}\n  got  {diff[0][1][:400]}"


def test_the_planner_reads_no_environment():
    """The planner's inputs are its arguments: no switch of its own from the process environment."""
    src = open(os.path.join(ROOT, "nyx_amd", "csrc", "launch_plan.h")).read()
    assert "getenv" not in src and "environ" not in src
