"""CPU: the host side of the targeter (nyx_amd/csrc/target_args.h: what the two entries refuse) and THE KERNELS' OWN per-run code
compiled for the host (nyx_amd/csrc/target_dev.h: the seed, the start states of a round, the step, the corrected state) as a
stand-alone C++ program with its own `main` (tests/cxx/target_host_check.cpp) - g++ only, no HIP, no GPU.  It is built twice with
-ffp-contract=off: plain, and with the address and undefined-behaviour sanitizers (their runtimes linked statically; nothing of it is
loaded into Python).  Both run the refusal table (every refusal of include/nyx_hip_target.h with its message, and which check wins),
then the cases of tests/target_cases.py: the program is fed the final states of every round of the definition on the CPU oracle as hex
floats and prints what the kernels would write - status, errors, total, the next 1 + V start states, the corrected state.  Against
nyx_amd/targeter.py every one of them is equal BIT FOR BIT (the objectives of the cases are formed with + - * / sqrt and fabs only)."""
import os
import subprocess

import numpy as np
import pytest

import target_cases as tc
from nyx_amd import _abi
from nyx_amd.targeter import target_definition

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cxx", "target_host_check.cpp")
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]}
NAMES = sorted(tc.CASES)


def hx(v):
    return float(v).hex()


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """(the input file, per case: the solution of the definition and the start and final states of its rounds): computed once."""
    base = tc.oracle_until_epoch(tc.two_body_compiled())
    lines, want = [str(len(NAMES))], []
    for name in NAMES:
        c = tc.CASES[name]
        calls = []

        def recording(batch, end_epoch_ns):
            out, st = base(batch, end_epoch_ns)
            calls.append((batch.rv(), out.rv(), np.asarray(st.status).copy()))
            return out, st
        V, O, iterations = len(c["variables"]), len(c["objectives"]), c.get("iterations", 100)
        sol = target_definition(recording, tc.batch_of(c["rv"]), c["variables"], c["objectives"], tc.EPOCH, tc.EPOCH + c["dur_ns"], tc.MU,
                                correction_frame=c.get("frame"), iterations=iterations)
        rounds = calls[1:]          # (call 0 is the leg to the correction epoch)
        assert len(rounds) == sol.iterations_run and all(r[0].shape == (1 + V, 6) for r in rounds)
        lines.append(f"{V} {O} {iterations} {_abi.FRAME_VNC if c.get('frame') == 'VNC' else _abi.FRAME_INERTIAL}")
        for v in c["variables"]:
            lines.append(" ".join([str(int(v.component))] + [hx(x) for x in (v.perturbation, v.init_guess, v.max_step, v.max_value, v.min_value)]))
        for o in c["objectives"]:
            lines.append(" ".join([str(int(o.parameter))] + [hx(x) for x in (o.desired_value, o.tolerance, o.multiplicative_factor, o.additive_factor)]))
        lines.append(hx(tc.MU))
        lines.append(" ".join(hx(x) for x in calls[0][1][0]))
        lines.append(str(len(rounds)))
        for _, final, status in rounds:
            for k in range(1 + V):
                lines.append(" ".join([str(int(status[k]))] + [hx(x) for x in final[k]]))
        want.append((name, sol, [r[0] for r in rounds]))
    path = tmp_path_factory.mktemp("target_host") / "input.txt"
    path.write_text("\n".join(lines) + "\n")
    return str(path), want


def same_bits(a, b):
    a, b = np.array(a, dtype=np.float64), np.array(b, dtype=np.float64)
    a[np.isnan(a)] = np.nan          # (a NaN's sign and payload are not part of the definition)
    b[np.isnan(b)] = np.nan
    return a.shape == b.shape and (a.view(np.uint64) == b.view(np.uint64)).all()


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_refusals_and_the_kernels_own_code_against_the_definition(world, tmp_path, build):
    path, want = world
    exe = str(tmp_path / f"target_host_check_{build}")
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", *BUILDS[build], "-Wall", "-Werror", SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)          # the refusal table alone
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "ok", r.stdout[-3000:] + r.stderr[-3000:]
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    out = [ln.split() for ln in r.stdout.strip().splitlines()]
    assert out[-1] == ["ok"]
    f = lambda toks: [float.fromhex(t) for t in toks]   # noqa: E731
    seen = set()
    for c, (name, sol, starts) in enumerate(want):
        case = tc.CASES[name]
        V, O = len(case["variables"]), len(case["objectives"])
        mine = [t for t in out if len(t) > 1 and t[1] == str(c) and t[0] in ("seed", "start", "step", "corrected")]
        seed = [t for t in mine if t[0] == "seed"][0]
        assert same_bits(f(seed[2:]), [v.init_guess for v in case["variables"]]), name
        # the start states of every round: what the definition handed to the propagator
        got_starts = {}
        for t in mine:
            if t[0] == "start":
                got_starts.setdefault(int(t[2]), []).append(f(t[4:10]))
        assert sorted(got_starts) == list(range(len(starts))), name
        for rnd, rows in got_starts.items():
            assert same_bits(rows, starts[rnd]), (name, rnd)
        steps = [t for t in mine if t[0] == "step"]
        assert [int(t[2]) for t in steps] == list(range(sol.iterations_run)) and [int(t[3]) for t in steps[:-1]] == [-1] * (len(steps) - 1), name
        last = steps[-1]
        assert int(last[3]) == int(sol.status[0]) == int(case["status"]) and int(last[2]) == int(sol.iterations[0]), name
        assert same_bits(f(last[4:4 + O]), sol.achieved_errors[:, 0]), name
        assert same_bits(f(last[4 + O:4 + O + V]), sol.correction[:, 0]), name
        corrected = [t for t in mine if t[0] == "corrected"]
        assert len(corrected) == 1 and same_bits(f(corrected[0][2:8]), sol.corrected.rv()[0]), name
        seen.add(int(sol.status[0]))
    assert seen == {0, 1, 2, 3, 4}          # CONVERGED, TOO_MANY_ITERATIONS, INEFFECTIVE, SINGULAR, NOT_FINITE
    print(f"{build}: {len(want)} cases, {sum(s.iterations_run for _, s, _ in want)} rounds, bit for bit")


def test_the_target_headers_read_no_environment_and_no_hip():
    for name in ("target_args.h", "target_dev.h"):
        src = open(os.path.join(ROOT, "nyx_amd", "csrc", name)).read()
        assert "getenv" not in src and "environ" not in src and "hip_runtime" not in src, name
