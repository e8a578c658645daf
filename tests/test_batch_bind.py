"""CPU: the batch binding (nyx_amd/csrc/batch_bind.h, used by abi.cpp) and the calibration fit (calibration_fit in launch_plan.h, used
by calibrate() in abi.cpp) as a stand-alone C++ check - g++ only, no HIP, no GPU.  The state-row table, bind_batch against written-out
DevBatch fields (refusals included), slices, shard bounds, the trajectory scatter and block layout, and the weight key of the
covariance-mapping loop; then calibrations replayed on synthetic cycle tables over the BASELINE shapes, every line equal to
tests/golden/calibration_fit.txt (written by the calibrate() of the commit before the fit moved out of abi.cpp, compiled on the host
with HIP stubbed and a fake launch that writes the same tables; the weights as hex floats)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "calibration_fit.txt")


def test_batch_bind_check(tmp_path):
    exe = str(tmp_path / "batch_bind_check")
    fits = str(tmp_path / "fits.txt")
    subprocess.run(["g++", "-std=c++17", "-O2", os.path.join(ROOT, "tests", "cxx", "batch_bind_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe, fits], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert r.stdout.strip().endswith("ok")
    assert "corner-case shapes differ" in r.stdout
    with open(fits) as f:
        got = f.read().splitlines()
    with open(GOLDEN) as f:
        want = f.read().splitlines()
    assert len(got) == len(want)
    diff = [(w, g) for w, g in zip(want, got) if w != g]
    assert not diff, f"{len(diff)} fits differ from the golden; first:\n  want {diff[0][0][:400]}\n  got  {diff[0][1][:400]}"


def test_the_batch_binding_reads_no_environment():
    """Host only: no environment, no HIP runtime."""
    src = open(os.path.join(ROOT, "nyx_amd", "csrc", "batch_bind.h")).read()
    assert "getenv" not in src and "environ" not in src and "hip_runtime" not in src
