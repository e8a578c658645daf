"""CPU: the host side of the sampled-series entries (nyx_amd/csrc/series_host.h, used by abi.cpp and the launchers of the four series
kernels) as a stand-alone C++ check - g++ only, no HIP, no GPU.  Every refusal of traj_at / traj_every and of the three fused reports
(return code, message, which check wins when two arguments are bad), every line equal to tests/golden/series_check.txt (written by
the check_traj, check_values_query, check_gt_query, check_ric_query and the argument checks of traj_eval_device of the commit before
they moved out of abi.cpp, compiled on the host with nyx_set_error capturing the message and run through the same case table,
tests/cxx/series_host_cases.h); the layout of the output block of the host flavours; the chunk planning of the launchers against the
expression they carried, around its seams (16 x 32768 samples and above: no GPU test can afford that shape)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "series_check.txt")


def test_series_host_check(tmp_path):
    exe = str(tmp_path / "series_host_check")
    refusals = str(tmp_path / "refusals.txt")
    subprocess.run(["g++", "-std=c++17", "-O2", os.path.join(ROOT, "tests", "cxx", "series_host_check.cpp"), "-o", exe], check=True)
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


def test_the_series_host_header_reads_no_environment():
    """Host only: no environment, no HIP runtime."""
    src = open(os.path.join(ROOT, "nyx_amd", "csrc", "series_host.h")).read()
    assert "getenv" not in src and "environ" not in src and "hip_runtime" not in src
