"""CPU: the host side of the statistics entries (nyx_amd/csrc/stats_host.h: the refusals, the kinds, the device block) and THE KERNEL'S
OWN per-value code compiled for the host (nyx_amd/csrc/stats_dev.h: the key map, who is held, the quantile formula, the summation
order) as a stand-alone C++ program with its own `main` (tests/cxx/stats_host_check.cpp) - g++ only, no HIP, no GPU.  Built twice with
-ffp-contract=off: plain, and with the address and undefined-behaviour sanitizers (their runtimes linked statically; nothing of it is
loaded into Python).  Both run the adversarial blocks of tests/stats_cases.py and print with `%a`.  Against nyx_amd/stats.py: the
integer columns, the extremes, SHIFT and every quantile BIT FOR BIT; SUM within FINITE * 2^-53 * sum |d| and SUMSQ within
FINITE * 2^-53 * sum d^2 of the fsum value (the program adds in the kernel's order: the classical bound of any order)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from nyx_amd import _abi
from nyx_amd import stats as st

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from stats_cases import adversarial_block, big_block, block_probs, compare  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cxx", "stats_host_check.cpp")
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]}


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """(the input file, the blocks): written once."""
    blocks = []
    for n in (1, 2, 63, 64, 65, 255, 256, 257, 1000):
        v, length, status = adversarial_block(n)
        blocks.append((v, length, status, block_probs(length, 5, 4, status if n % 2 == 1 else None), n % 2 == 1))
    v, length, status = big_block(3000)
    blocks.append((v, length, status, (0.01, 0.5, 0.99), True))
    blocks.append((np.zeros((2, 3, 0)), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32), (0.5,), False))
    lines = [str(len(blocks))]
    for v, length, status, probs, with_status in blocks:
        lines.append(f"{v.shape[0]} {v.shape[1]} {v.shape[2]} {len(probs)} {int(with_status)}")
        lines.append(" ".join(float(p).hex() for p in probs))
        lines.append(" ".join(str(int(x)) for x in length))
        lines.append(" ".join(str(int(x)) for x in status))
        lines.append(" ".join(float(x).hex() for x in v.ravel()))
    path = tmp_path_factory.mktemp("stats_host") / "input.txt"
    path.write_text("\n".join(lines) + "\n")
    return str(path), blocks


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_the_kernels_own_code_on_the_host_agrees_with_the_definition(cases, build, tmp_path):
    path, blocks = cases
    exe = str(tmp_path / f"stats_host_check_{build}")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *BUILDS[build], SRC, "-o", exe], check=True)
    run = subprocess.run([exe, path], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    lines = run.stdout.splitlines()
    at = 0
    for v, length, status, probs, with_status in blocks:
        rows, cap, n = v.shape
        got = np.array([[float.fromhex(w) for w in lines[at + k].split()] for k in range(rows * cap)]).reshape(rows, cap, 10 + len(probs))
        at += rows * cap
        stt = status if with_status else None
        compare(got, st.series_stats(v, length, probs, status=stt), v, length, stt, f"{build}, n = {n}")
    assert lines[at] == "REFUSALS"
    vq, lq = C.sizeof(_abi.ValuesQuery), C.sizeof(_abi.LinkQuery)
    want = ["0|", "1|null ctx", "1|series_stats: null statistics query", "1|series_stats: n_probs = 9, 0 .. 8 probabilities per call",
            "1|series_stats: n_probs = -1, 0 .. 8 probabilities per call", "1|series_stats: prob[0] must lie in [0, 1]", "1|series_stats: prob[0] must lie in [0, 1]",
            "1|series_stats: prob[0] must lie in [0, 1]", "1|series_stats: n_rows must be >= 1", "1|series_stats: capacity must be 1 .. 2^31 - 1",
            "1|series_stats: capacity must be 1 .. 2^31 - 1", "1|series_stats: n must be 0 .. 2^31 - 1", "1|series_stats: stats array required",
            "1|series_stats: values and len arrays required", "1|series_stats: values and len arrays required", "0|",
            "0|", "1|null ctx", "1|traj_series_stats: kind = 7 is not a nyx_hip_series_kind", "1|traj_series_stats: null traj", "1|traj_series_stats: null query",
            f"1|traj_series_stats: query_size = {vq - 8}, the query of traj_values is {vq} bytes", "1|traj_series_stats: traj_values takes no second batch (ref)",
            "1|traj_series_stats: traj_link needs a second batch (ref)", "0|", "1|traj_series_stats: prob[0] must lie in [0, 1]",
            "1|traj_series_stats: stats and len arrays required", "1|traj_series_stats: stats and len arrays required",
            "rows 5 12 6"]
    assert lines[at + 1:at + 1 + len(want)] == want
    kinds = lines[at + 1 + len(want):at + 8 + len(want)]
    sizes = [C.sizeof(q) for q in (_abi.ValuesQuery, _abi.GtQuery, _abi.AerQuery, _abi.EclQuery, _abi.FrameQuery, _abi.LinkQuery, _abi.RicQuery)]
    names = sorted(_abi.SERIES_KINDS, key=_abi.SERIES_KINDS.get)
    assert kinds == [f"kind {k} {sizes[k]} {int(k >= 5)} {names[k]}" for k in range(7)] and lq == sizes[5]
    values, stats = 8 * 91 * 10000 * 8, 8 * 91 * 13 * 8                       # the headline ensemble: 58 MB of values, 76 KB of statistics
    assert lines[-1] == f"block 0 {values} {values} {stats} {values + stats} 40000 {values + stats + 40000} 40000 {values + stats + 80000}"
