"""CPU: the host side of the entries that run the propagator (nyx_amd/csrc/run_host.h and the launch predicates beside pick_quad in
launch_plan.h, used by abi.cpp) as a stand-alone C++ check - g++ only, no HIP, no GPU.  Every refusal of propagate_batch /
_with_traj / until_epoch / _sharded, until_event, predict_until, ensemble_moments (both flavours) and the host flavour of traj_at /
traj_every (return code, message, which check wins when two arguments are bad, an empty batch with bad later arguments), every line
equal to tests/golden/run_check.txt (written by the checks those entries carried inline in abi.cpp in the commit before they moved
out, copied into a host program with nyx_set_error capturing the message and run through the same case table,
tests/cxx/run_host_cases.h); the device blocks of predict_until, until_event and ensemble_moments against the allocations they
replace; the segments of a covariance-mapping loop and the three launch predicates against the expressions abi.cpp carried."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "run_check.txt")


def test_run_host_check(tmp_path):
    exe = str(tmp_path / "run_host_check")
    refusals = str(tmp_path / "refusals.txt")
    subprocess.run(["g++", "-std=c++17", "-O2", os.path.join(ROOT, "tests", "cxx", "run_host_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe, refusals], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert r.stdout.strip().endswith("ok")
    with open(refusals) as f:
        got = f.read().splitlines()
    with open(GOLDEN) as f:
        want = f.read().splitlines()
    assert len(got) == len(want)
    diff = [(w, g) for w, g in zip(want, got) if w != g]
    assert not diff, f"{len(diff)} cases differ from the golden; first:\n  want {diff[0][0]}\n  got  {diff[0][1]}"


def test_the_run_host_header_reads_no_environment():
    """Host only: no environment, no HIP runtime."""
    src = open(os.path.join(ROOT, "nyx_amd", "csrc", "run_host.h")).read()
    assert "getenv" not in src and "environ" not in src and "hip_runtime" not in src
