"""CPU: the host side of the encounter report (nyx_amd/csrc/series_host.h: `check_frame_series`, `check_frame_context`;
nyx_amd/csrc/frame_args.h: the needs of the parameters, the reduction of the chain) and THE KERNEL'S OWN per-sample code compiled for
the host (nyx_amd/csrc/frame_dev.h: the Clenshaw recurrence with its derivative, the shared intermediates, the B-plane, the 25
parameters) as a stand-alone C++ program with its own `main` (tests/cxx/frame_host_check.cpp) - g++ only, no HIP, no GPU.  It is built
twice with -ffp-contract=off: plain, and with the address and undefined-behaviour sanitizers (their runtimes linked statically: the
program does not depend on which libraries the loader brings in first; nothing of it is loaded into Python).  Both run the refusals
over a table of cases (every refusal of include/nyx_hip_frame.h with its message, and which check wins) and the reduction over
hand-made chains, then evaluate the almanac of the tests - its records laid out packed AND sixteen coefficients wide - at a few
hundred (target, epoch, state) cases and print with `%a`.  Against nyx_amd/frames.py: the body's position and velocity BIT FOR BIT in
both layouts and both builds (the position also when the velocity recurrence is skipped); the parameters formed with + - * / sqrt
only BIT FOR BIT, those through atan2 / acos / pow within 2 ulp (both sides use this C library, numpy possibly its own vector code)."""
import json
import os
import subprocess

import numpy as np
import pytest

import nyx_amd as nx
from nyx_amd import eclipse, ephem, frames
from nyx_amd.frames import FrameParameter as F
from scenarios import EPOCH0_NS, leo_full_setup, leo_nominal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cxx", "frame_host_check.cpp")
LIBM = (F.Inclination, F.RAAN, F.AoP, F.TrueAnomaly, F.Period, F.BAngle)
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]}


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """(the input file, the cases, what frames.py gives for them): written and computed once."""
    prop, almanac, central = leo_full_setup(degree=0)
    targets = [central] + [almanac.frame_info(b) for b in (nx.MOON, nx.SUN, nx.JUPITER_BARYCENTER)]
    davis = np.array(json.load(open(os.path.join(ROOT, "tests", "golden", "bplane_davis.json")))["state_km_km_s"])
    rng = np.random.default_rng(17)
    cases = []
    for t, target in enumerate(targets):
        segs = [almanac.segments[s] for s, _ in eclipse.body_chain(target.naif_id, almanac, central)] or list(almanac.segments)
        t0 = max(float(s.init_et_s) for s in segs)
        t1 = min(float(s.init_et_s) + float(s.interval_s) * s.records.shape[0] for s in segs)
        epochs = np.concatenate([np.linspace(int(np.ceil(t0 * 1e9)), int(round(t1 * 1e9)), 60).astype(np.int64),
                                 [int(round(t1 * 1e9)), EPOCH0_NS, EPOCH0_NS + 4321 * 10**9 + 987654321, int(round(t1 * 1e9)) + 10**9]])
        for k, ep in enumerate(epochs):
            rv = davis if k % 8 == 3 else leo_nominal() + rng.standard_normal(6) * np.array([50.0, 50.0, 50.0, 0.05, 0.05, 0.05])
            cases.append((t, int(ep), np.array(rv, dtype=np.float64)))
    lines = [str(len(almanac.segments))]
    for seg in almanac.segments:
        rec = np.asarray(seg.records, dtype=np.float64)
        lines.append(f"{float(seg.init_et_s).hex()} {float(seg.interval_s).hex()} {rec.shape[0]} {seg.n_coeffs}")
        lines.append(" ".join(float(v).hex() for v in rec.ravel()))
    lines.append(str(len(targets)))
    for target in targets:
        chain = eclipse.body_chain(target.naif_id, almanac, central)
        lines.append(" ".join([float(target.mu_km3_s2).hex(), str(len(chain))] + [f"{s} {g}" for s, g in chain]))
    lines.append(str(len(cases)))
    for t, ep, rv in cases:
        lines.append(" ".join([str(t), float(frames._ns_to_seconds(np.int64(ep))).hex()] + [float(v).hex() for v in rv]))
    path = tmp_path_factory.mktemp("frame_host") / "input.txt"
    path.write_text("\n".join(lines) + "\n")
    body, vals = [], []
    for t, ep, rv in cases:
        r, v = frames.body_state(targets[t].naif_id, np.int64(ep), almanac, central)
        body.append(np.concatenate([r, v]))
        vals.append([float(frames.frame_value(p, rv, np.int64(ep), targets[t], almanac, central)) for p in F])
    return str(path), cases, np.array(body), np.array(vals), targets


def same_bits(a, b):
    return (np.asarray(a, dtype=np.float64).view(np.uint64) == np.asarray(b, dtype=np.float64).view(np.uint64)).all()


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_refusals_reduction_and_the_kernels_own_code_against_the_definition(world, tmp_path, build):
    path, cases, body, vals, targets = world
    assert len(cases) == 4 * 64
    exe = str(tmp_path / f"frame_host_check_{build}")
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", *BUILDS[build], "-Wall", "-Werror", SRC, "-o", exe], check=True)
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    out = r.stdout.strip().splitlines()
    assert out[-1] == "ok"
    n_body = n_slim = n_val = 0
    worst = 0.0
    outside = set()
    for ln in out[:-1]:
        tok = ln.split()
        layout, c = int(tok[1]), int(tok[2])
        nan_row = np.isnan(body[c]).all()
        if tok[0] in ("body", "slim"):
            width = 6 if tok[0] == "body" else 3
            got, st = np.array([float.fromhex(t) for t in tok[3:3 + width]]), int(tok[3 + width])
            assert (st != 0) == nan_row, (ln, body[c])       # NYX_HIP_ERR_EPHEM_RANGE exactly where the definition has a row of NaN
            if nan_row:
                outside.add(cases[c][0])
            else:
                assert same_bits(got, body[c][:width]), (tok[0], layout, c, got, body[c])
            n_body, n_slim = n_body + (tok[0] == "body"), n_slim + (tok[0] == "slim")
            continue
        assert tok[0] == "val"
        p, got, alone = F(int(tok[3])), float.fromhex(tok[4]), float.fromhex(tok[5])
        assert same_bits(got, alone), (p, layout, c)          # the shared intermediates of all 25, or of this parameter alone
        n_val += 1
        if nan_row:
            continue                                           # (the kernel never uses the values of a sample outside the ephemerides)
        want = vals[c][int(p)]
        assert np.isnan(got) == np.isnan(want), (p, layout, c, got, want)
        if np.isnan(want):
            continue
        if p in LIBM:
            ulps = abs(got - want) / np.spacing(abs(want))
            worst = max(worst, ulps)
            assert ulps <= 2.0, (p, layout, c, got, want)
        else:
            assert same_bits(got, want), (p, layout, c, got.hex(), float(want).hex())
    assert n_body == n_slim == 2 * len(cases) and n_val == 2 * len(cases) * 25      # both layouts
    assert outside == {1, 2, 3}                                                      # every chain was asked past its end; the centre has none
    # the cases reach both kinds of orbit about a target, with and without a translation
    hyp = np.isfinite(vals[:, int(F.BdotT)])
    for t, (some_hyperbolic, some_not) in enumerate([(True, True), (True, False), (False, True), (True, False)]):   # Earth, Moon, Sun, Jupiter
        mine = np.array([c[0] == t for c in cases]) & ~np.isnan(body).all(axis=1)
        assert hyp[mine].any() == some_hyperbolic and (~hyp[mine]).any() == some_not, t
    print(f"{build}: libm parameters within {worst:.2f} ulp")


def test_the_frame_headers_read_no_environment_and_no_hip():
    for name in ("frame_args.h", "frame_dev.h"):
        src = open(os.path.join(ROOT, "nyx_amd", "csrc", name)).read()
        assert "getenv" not in src and "environ" not in src and "hip_runtime" not in src, name
    assert ephem.MU_EARTH > 0
