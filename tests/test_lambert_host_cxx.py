"""CPU: the host side of the Lambert transfers (nyx_amd/csrc/lambert_args.h: what the two entries refuse) and THE KERNELS' OWN per-problem
code compiled for the host (nyx_amd/csrc/lambert_dev.h: the solver, the status rules, the sixteen parameters, a body's state about the
centre) as a stand-alone C++ program with its own `main` (tests/cxx/lambert_host_check.cpp) - g++ only, no HIP, no GPU.  It is built
twice with -ffp-contract=off: plain, and with the address and undefined-behaviour sanitizers (their runtimes linked statically; nothing
of it is loaded into Python).  Both run the refusal table (every refusal of include/nyx_hip_lambert.h with its message, and which check
wins), then the seeded problems of tests/lambert_cases.py under every way, revolution count and path, and cells of an Earth -> Jupiter
grid about the Sun - the almanac's records laid out packed AND sixteen coefficients wide - printing with `%a`.  Against
nyx_amd/lambert.py: `status` and Iterations equal, the body states BIT FOR BIT in both layouts, the values within the bounds of
tests/test_gpu_lambert.py (both sides call this C library: in fact the same bits, which is asserted for the solver's own arithmetic)."""
import os
import subprocess

import numpy as np
import pytest

import nyx_amd as nx
from nyx_amd import lambert
from nyx_amd.frames import _ns_to_seconds
from nyx_amd.lambert import LambertParameter as P, LambertStatus as St
from lambert_cases import MARGIN, MU_EARTH, bounds, problems
from scenarios import EPOCH0_NS, leo_full_setup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cxx", "lambert_host_check.cpp")
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]}
SETTINGS = [(way, m, hp, 1000, 1e-4) for way in (0, 1, 2) for m, hp in ((0, 0), (1, 0), (1, 1), (2, 0), (2, 1))] + [(0, 0, 0, 2, 1e-10)]
DAY = 86400 * 10**9


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """(the input file, the problems and cells, what lambert.py gives for them): written and computed once."""
    prop, almanac, central = leo_full_setup(degree=0)
    earth, jupiter, sun = (almanac.frame_info(b) for b in (central.naif_id, nx.JUPITER_BARYCENTER, nx.SUN))
    rv1, rv2, tof = problems()
    lines = [str(len(almanac.segments))]
    for seg in almanac.segments:
        rec = np.asarray(seg.records, dtype=np.float64)
        lines.append(f"{float(seg.init_et_s).hex()} {float(seg.interval_s).hex()} {rec.shape[0]} {seg.n_coeffs}")
        lines.append(" ".join(float(v).hex() for v in rec.ravel()))
    for body in (earth, jupiter, sun):
        chain = lambert.check_chain("body", body.naif_id, almanac, central)
        lines.append(" ".join([str(len(chain))] + [f"{s} {g}" for s, g in chain]))
    want = []
    lines.append(str(len(SETTINGS) * rv1.shape[1]))
    for way, m, hp, max_iter, tol in SETTINGS:
        values, status, extras = lambert.batch_definition(rv1, rv2, tof, MU_EARTH, way, m, hp, tol, max_iter)
        want.append((values, status, extras))
        for i in range(rv1.shape[1]):
            lines.append(" ".join([str(way), str(m), str(hp), str(max_iter), float(tol).hex(), float(MU_EARTH).hex()] + [float(v).hex() for v in rv1[:, i]]
                                  + [float(v).hex() for v in rv2[:, i]] + [float(tof[i]).hex()]))
    # cells: a 6 x 9 grid inside the table, and a row and a column outside it
    dep_ns, arr_ns = lambert.grid_epochs(7, 10, EPOCH0_NS - 30 * DAY, 6 * DAY, arr0_ns=EPOCH0_NS + 8 * DAY, arr_step_ns=4 * DAY)
    g_values, g_status, g_extras, _, _ = lambert.grid_definition(earth, jupiter, sun, almanac, central, 7, 10, EPOCH0_NS - 30 * DAY, 6 * DAY,
                                                                 arr0_ns=EPOCH0_NS + 8 * DAY, arr_step_ns=4 * DAY)
    g_rv1, g_rv2, inside = lambert.grid_states(earth, jupiter, sun, dep_ns, arr_ns, almanac, central)
    mu = float(sun.mu_km3_s2)
    lines.append(str(70))
    for i in range(7):
        for j in range(10):
            lines.append(" ".join(float(v).hex() for v in (_ns_to_seconds(dep_ns[i]), _ns_to_seconds(arr_ns[i, j]), _ns_to_seconds(arr_ns[i, j] - dep_ns[i]), mu)))
    path = tmp_path_factory.mktemp("lambert_host") / "input.txt"
    path.write_text("\n".join(lines) + "\n")
    return str(path), (rv1, rv2, tof), want, (g_values, g_status, g_extras, g_rv1, g_rv2, inside)


def same_bits(a, b):
    return (np.asarray(a, dtype=np.float64).view(np.uint64) == np.asarray(b, dtype=np.float64).view(np.uint64)).all()


def held(label, got, want, status, extras, rv1, rv2):
    """status equal; where solved: decision_margin wide, Iterations equal, every value inside its bound; NaN elsewhere"""
    solved = status == St.OK
    assert (np.array([e["decision_margin"] for e in extras])[solved] >= MARGIN).all(), label
    assert np.isnan(got[:, ~solved]).all() and np.isfinite(got[:, solved]).all(), label
    np.testing.assert_array_equal(got[P.Iterations][solved], want[P.Iterations][solved], err_msg=label)
    b = bounds(want, extras, rv1, rv2)
    d = np.abs(got[:, solved] - want[:, solved])
    assert (d <= b[:, solved]).all(), (label, float(np.max(d / np.maximum(b[:, solved], 1e-300))))
    return float(np.max(np.where(b[:, solved] > 0.0, d / np.where(b[:, solved] > 0.0, b[:, solved], 1.0), 0.0))) if solved.any() else 0.0


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_refusals_and_the_kernels_own_code_against_the_definition(world, tmp_path, build):
    path, (rv1, rv2, tof), want, (g_values, g_status, g_extras, g_rv1, g_rv2, inside) = world
    exe = str(tmp_path / f"lambert_host_check_{build}")
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", *BUILDS[build], "-Wall", "-Werror", SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)          # the refusal table alone
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "ok", r.stdout[-3000:] + r.stderr[-3000:]
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    out = r.stdout.strip().splitlines()
    assert out[-1] == "ok"
    n = rv1.shape[1]
    sol = [ln.split() for ln in out if ln.startswith("sol ")]
    assert len(sol) == len(SETTINGS) * n
    worst, seen = 0.0, set()
    for k, (values, status, extras) in enumerate(want):
        rows = sol[k * n:(k + 1) * n]
        assert [int(t[1]) for t in rows] == list(range(k * n, (k + 1) * n))
        got_status = np.array([int(t[2]) for t in rows])
        got = np.array([[float.fromhex(v) for v in t[3:19]] for t in rows]).T
        np.testing.assert_array_equal(got_status, status, err_msg=str(SETTINGS[k]))
        worst = max(worst, held(str(SETTINGS[k]), got, values, status, extras, rv1, rv2))
        seen |= set(status.tolist())
    assert seen == {St.OK, St.BAD_INPUT, St.DEGENERATE, St.NOT_FEASIBLE, St.TOO_CLOSE, St.MAX_ITER}
    cells = [ln.split() for ln in out if ln.startswith("cell ")]
    assert len(cells) == 2 * 70
    flat_rv1 = np.broadcast_to(g_rv1[:, None, :], g_rv2.shape).reshape(-1, 6)
    flat_rv2, flat_in, flat_status = g_rv2.reshape(-1, 6), inside.reshape(-1), g_status.reshape(-1)
    assert (flat_status == St.EPHEM_RANGE).sum() >= 10 and (flat_status == St.OK).sum() >= 40 and ((flat_status == St.EPHEM_RANGE) == ~flat_in).all()
    for layout in (0, 1):
        rows = cells[layout * 70:(layout + 1) * 70]
        assert [(int(t[1]), int(t[2])) for t in rows] == [(layout, c) for c in range(70)]
        got = np.array([[float.fromhex(v) for v in t[18:34]] for t in rows]).T
        for c, t in enumerate(rows):
            st1, st2, st = int(t[3]), int(t[10]), int(t[17])
            b1, b2 = [float.fromhex(v) for v in t[4:10]], [float.fromhex(v) for v in t[11:17]]
            assert st == flat_status[c] and ((st1 != 0) or (st2 != 0)) == (not flat_in[c]), (layout, c)
            if st1 == 0:
                assert same_bits(b1, flat_rv1[c]), (layout, c, b1, flat_rv1[c])
            if st2 == 0:
                assert same_bits(b2, flat_rv2[c]), (layout, c, b2, flat_rv2[c])
        worst = max(worst, held(f"cells layout {layout}", got, g_values.reshape(16, -1), flat_status, [e for row in g_extras for e in row], flat_rv1.T, flat_rv2.T))
    timing = [ln.split() for ln in out if ln.startswith("time ")]
    assert len(timing) == 1 and float(timing[0][1]) > 0.0
    print(f"{build}: worst deviation {worst:.3f} of its bound; {float(timing[0][1]):.0f} ns per solve on one core over {timing[0][2]} solves")


def test_the_lambert_headers_read_no_environment_and_no_hip():
    for name in ("lambert_args.h", "lambert_dev.h"):
        src = open(os.path.join(ROOT, "nyx_amd", "csrc", name)).read()
        assert "getenv" not in src and "environ" not in src and "hip_runtime" not in src, name
