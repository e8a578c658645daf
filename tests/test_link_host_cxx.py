"""CPU: the host side of the link report (nyx_amd/csrc/series_host.h: `check_link_series`, `check_link_context`;
nyx_amd/csrc/link_args.h: the needs of the parameters, the reduction of the chains) and THE KERNEL'S OWN per-sample code compiled for the
host (nyx_amd/csrc/link_dev.h: the segments of a sample, the SIGHT test, the twelve parameters) as a stand-alone C++ program with its own
`main` (tests/cxx/link_host_check.cpp) - g++ only, no HIP, no GPU.  It is built twice with -ffp-contract=off: plain, and with the
address and undefined-behaviour sanitizers (their runtimes linked statically: the program does not depend on which libraries the
loader brings in first; nothing of it is loaded into Python).  Both run the refusals over a table of cases (every refusal of
include/nyx_hip_link.h with its message, and which check wins) and the reduction over hand-made chains, then evaluate the almanac of the
tests - its records laid out packed AND sixteen coefficients wide - at a few hundred (epoch, receiver, transmitter) cases against the
Earth, the Moon and the Sun and print with `%a`.  Against nyx_amd/links.py: all twelve parameters BIT FOR BIT in both layouts and both
builds (only + - * / sqrt and comparisons on either side)."""
import os
import subprocess

import numpy as np
import pytest

import nyx_amd as nx
from nyx_amd import eclipse, links
from nyx_amd.groundtrack import _ns_to_seconds
from nyx_amd.links import LinkParameter as L
from scenarios import EPOCH0_NS, leo_full_setup, leo_nominal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cxx", "link_host_check.cpp")
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]}
RETRO = np.array([1.0, 1.0, 1.0, -1.0, -1.0, -1.0])


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """(the input file, the cases, what links.py gives for them): written and computed once."""
    prop, almanac, central = leo_full_setup(degree=0)
    bodies = [central, almanac.frame_info(nx.MOON), almanac.frame_info(nx.SUN)]
    segs = list(almanac.segments)
    t0 = max(float(s.init_et_s) for s in segs)
    t1 = min(float(s.init_et_s) + float(s.interval_s) * s.records.shape[0] for s in segs)
    epochs = np.concatenate([np.linspace(int(np.ceil(t0 * 1e9)), int(round(t1 * 1e9)) - 10**9, 250).astype(np.int64),
                             [EPOCH0_NS, EPOCH0_NS + 4321 * 10**9 + 987654321, int(round(t1 * 1e9)) + 10**12, int(np.ceil(t0 * 1e9)) - 10**12]])
    rng = np.random.default_rng(23)
    cases = []
    for k, ep in enumerate(epochs):
        rx = leo_nominal() + rng.standard_normal(6) * np.array([50.0, 50.0, 50.0, 0.05, 0.05, 0.05])
        tx = leo_nominal() * RETRO + rng.standard_normal(6) * np.array([50.0, 50.0, 50.0, 0.05, 0.05, 0.05])
        if k % 4 == 1:                                   # opposite sides of the Earth
            tx[:3] = -rx[:3] + rng.standard_normal(3) * 300.0
        elif k % 4 == 2:                                 # the two sides of the Moon
            pm = eclipse.body_position(nx.MOON, np.int64(ep), almanac, central)
            if not np.isnan(pm).any():
                side = np.cross(pm, rng.standard_normal(3))
                side *= 4000.0 / np.linalg.norm(side)
                rx[:3], tx[:3] = pm + side + rng.standard_normal(3) * 900.0, pm - side + rng.standard_normal(3) * 900.0
        elif k % 16 == 3:                                # coincident
            tx = rx.copy()
        cases.append((int(ep), rx, tx))
    lines = [str(len(segs))]
    for seg in segs:
        rec = np.asarray(seg.records, dtype=np.float64)
        lines.append(f"{float(seg.init_et_s).hex()} {float(seg.interval_s).hex()} {rec.shape[0]} {seg.n_coeffs}")
        lines.append(" ".join(float(v).hex() for v in rec.ravel()))
    lines.append(str(len(bodies)))
    for frame in bodies:
        chain = links.link_chain(frame, almanac, central)
        lines.append(" ".join([float(frame.mean_equatorial_radius_km).hex(), str(len(chain))] + [f"{s} {g}" for s, g in chain]))
    lines.append(str(len(cases)))
    for ep, rx, tx in cases:
        lines.append(" ".join([float(_ns_to_seconds(np.int64(ep))).hex()] + [float(v).hex() for v in np.concatenate([rx, tx])]))
    path = tmp_path_factory.mktemp("link_host") / "input.txt"
    path.write_text("\n".join(lines) + "\n")
    ep = np.array([c[0] for c in cases], dtype=np.int64)
    rx, tx = np.array([c[1] for c in cases]), np.array([c[2] for c in cases])
    want = {}
    for p in L:
        for b in (range(3) if p in links.PER_BODY else [-1]):
            want[(int(p), b)] = links.link_value(p, rx, tx, ep, bodies, almanac, central, body=None if b < 0 else b)
    outside = links.outside_ephemerides(ep, bodies, almanac, central)
    return str(path), cases, want, outside


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_refusals_reduction_and_the_kernels_own_code_against_the_definition(world, tmp_path, build):
    path, cases, want, outside = world
    assert len(cases) == 254 and outside.sum() == 2
    exe = str(tmp_path / f"link_host_check_{build}")
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", *BUILDS[build], "-Wall", "-Werror", SRC, "-o", exe], check=True)
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    out = r.stdout.strip().splitlines()
    assert out[-1] == "ok"
    seen = 0
    for ln in out[:-1]:
        tok = ln.split()
        assert tok[0] == "val"
        layout, c, p, b, got, st = int(tok[1]), int(tok[2]), int(tok[3]), int(tok[4]), float.fromhex(tok[5]), int(tok[6])
        seen += 1
        assert (st != 0) == bool(outside[c]), ln                # NYX_HIP_ERR_EPHEM_RANGE exactly where the definition says so
        if st != 0:
            continue                                           # (the kernel never uses the values of a sample outside the ephemerides)
        w = float(want[(p, b)][c])
        assert np.isnan(got) == np.isnan(w), (L(p).name, b, layout, c, got, w)
        if not np.isnan(w):
            assert np.float64(got).view(np.uint64) == np.float64(w).view(np.uint64), (L(p).name, b, layout, c, got.hex(), w.hex())
    # both layouts x two queries of eight; LosY and LosZ are in both queries
    assert seen == 2 * 16 * len(cases)
    # the cases reach every answer: the Earth obstructs, the Moon obstructs, nothing does; coincident pairs give NaN
    inside = ~outside
    first = want[(int(L.ObstructingBody), -1)][inside]
    assert {-1.0, 0.0, 1.0} == set(first.tolist()) and min((first == v).sum() for v in (-1.0, 0.0, 1.0)) >= 30
    assert np.isnan(want[(int(L.RangeRate), -1)]).sum() >= 10 and np.isnan(want[(int(L.BodyClearance), 2)][inside]).sum() >= 10
    assert (want[(int(L.BodyObstructs), 2)][inside] == 0.0).all()                  # (the Sun never does)


def test_the_link_headers_read_no_environment_and_no_hip():
    for name in ("link_args.h", "link_dev.h"):
        src = open(os.path.join(ROOT, "nyx_amd", "csrc", name)).read()
        assert "getenv" not in src and "environ" not in src and "hip_runtime" not in src, name
    # one copy of the per-sample code: the kernel calls what the program above ran
    kernel = open(os.path.join(ROOT, "nyx_amd", "csrc", "link_kernel.hip")).read()
    assert "lnk_sample(a, rx, tx," in kernel and "lnk_segments(a, ns_to_seconds(epoch)," in kernel and '#include "link_dev.h"' in kernel
