"""CPU: the host side of the eclipse report (nyx_amd/csrc/series_host.h: `check_ecl_series`; nyx_amd/csrc/eclipse_args.h: the needs of
the parameters, the reduction of the chains to their distinct segments) and THE KERNEL'S OWN per-sample code compiled for the host
(nyx_amd/csrc/eclipse_dev.h: the Clenshaw recurrence, the disk overlap) as a stand-alone C++ program with its own `main`
(tests/cxx/eclipse_host_check.cpp) - g++ only, no HIP, no GPU - built with the address and undefined-behaviour sanitizers (their
runtimes linked statically: the program does not depend on which libraries the loader brings in first).  It runs
`check_ecl_series` over a table of cases (every refusal of include/nyx_hip_eclipse.h with its message, and which check wins), the
reduction over hand-made chains (the Earth -> EMB segment shared by the Sun's and the Moon's chains counted once, chain order kept),
then evaluates the almanac of the tests - its records laid out packed AND sixteen coefficients wide, as the context builder may
lay them out - at the states this test hands it and prints positions and percentages with `%a`.  Those must equal the oracle's
(`nyx_oracle_body_position`, `nyx_oracle_occultation_factor`) BIT FOR BIT, in both layouts, and the states must reach all four
branches of the overlap formula."""
import ctypes as C
import os
import subprocess

import numpy as np

import nyx_amd as nx
import oracle_lib
from nyx_amd import _abi, eclipse
from scenarios import EPOCH0_NS, leo_full_setup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cases(almanac, central):
    """(epoch_ns, r): the Earth's penumbra, day side and umbra, the Moon's four branches, a state inside the Earth, two epochs."""
    out = []
    for ep in (EPOCH0_NS, EPOCH0_NS + 4321 * 10**9 + 987654321):
        p_sun = eclipse.body_position(nx.SUN, np.int64(ep), almanac, central)
        p_moon = eclipse.body_position(nx.MOON, np.int64(ep), almanac, central)
        shat = p_sun / np.linalg.norm(p_sun)
        perp = np.cross(shat, [0, 0, 1.0])
        perp /= np.linalg.norm(perp)
        for d in np.linspace(6300.0, 6460.0, 41):
            out.append((ep, -7000.0 * shat + d * perp))
        out += [(ep, 7000.0 * shat + 3.0 * perp), (ep, -7000.0 * shat + 3.0 * perp), (ep, -3000.0 * shat + 3.0 * perp)]
        u = p_moon - p_sun
        u /= np.linalg.norm(u)
        mperp = np.cross(u, [0, 0, 1.0])
        mperp /= np.linalg.norm(mperp)
        for d, off in [(5000.0, 3.0), (5000.0, 1725.0), (5000.0, 1800.0), (450000.0, 3.0), (450000.0, 3500.0)]:
            out.append((ep, p_moon + d * u + off * mperp))
    return out


def test_refusals_reduction_and_the_kernels_own_code_against_the_oracle(tmp_path):
    exe = str(tmp_path / "eclipse_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                    "-static-libubsan", "-Wall",
                    "-Werror", os.path.join(ROOT, "tests", "cxx", "eclipse_host_check.cpp"), "-o", exe], check=True)
    prop, almanac, central = leo_full_setup(degree=0)
    compiled = prop.compile(almanac, central)
    bodies = [nx.SUN, nx.EARTH, nx.MOON]          # the light source first
    cases = _cases(almanac, central)
    lines = [str(len(almanac.segments))]
    for seg in almanac.segments:
        rec = np.asarray(seg.records, dtype=np.float64)
        lines.append(f"{float(seg.init_et_s).hex()} {float(seg.interval_s).hex()} {rec.shape[0]} {seg.n_coeffs}")
        lines.append(" ".join(float(v).hex() for v in rec.ravel()))
    lines.append(str(len(bodies)))
    for naif in bodies:
        chain = eclipse.body_chain(naif, almanac, central)
        lines.append(" ".join([float(almanac.bodies[naif]["radius"]).hex(), str(len(chain))] + [f"{s} {g}" for s, g in chain]))
    lines.append(str(len(cases)))
    for ep, r in cases:
        lines.append(" ".join([str(int(ep))] + [float(v).hex() for v in r]))
    src = tmp_path / "input.txt"
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(src)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    out = r.stdout.strip().splitlines()
    assert out[-1] == "ok"

    lib = oracle_lib.load()
    index = {int(compiled.cfg.bodies[b].naif_id): b for b in range(compiled.cfg.n_bodies)}
    pos, st = np.zeros(3), C.c_int32()
    n_pos = n_pct = 0
    branches = set()
    for ln in out[:-1]:
        tok = ln.split()
        layout, c, b = int(tok[1]), int(tok[2]), int(tok[3])
        ep, rr = cases[c]
        if tok[0] == "pos":
            lib.nyx_oracle_body_position(C.byref(compiled.cfg), index[bodies[b]], int(ep), pos.ctypes.data_as(_abi.c_double_p), C.byref(st))
            assert st.value == 0 == int(tok[7])
            assert [float.fromhex(t).hex() for t in tok[4:7]] == [float(v).hex() for v in pos], (layout, c, b)
            n_pos += 1
        else:
            assert tok[0] == "pct"
            rr = np.ascontiguousarray(rr)
            want = lib.nyx_oracle_occultation_factor(C.byref(compiled.cfg), index[bodies[b]], index[nx.SUN], int(ep), rr.ctypes.data_as(_abi.c_double_p),
                                                     C.byref(st))
            assert st.value == 0
            assert float.fromhex(tok[5]).hex() == float(want).hex(), (layout, c, b, tok)
            # and the numpy definition gives the percentage itself, bit for bit
            mine = nx.eclipse_value(nx.EclipseParameter.BodyOccultation, rr, ep, nx.ShadowModel.cislunar(almanac), almanac, central, body=b - 1)
            assert float.fromhex(tok[4]).hex() == float(mine).hex(), (layout, c, b, tok)
            branches.add(tok[6])
            n_pct += 1
    assert n_pos == 2 * len(cases) * 3 and n_pct == 2 * len(cases) * 2      # both layouts
    assert branches == {"lit", "umbra", "penumbra", "annular"}


def test_the_eclipse_headers_read_no_environment_and_no_hip():
    for name in ("eclipse_args.h", "eclipse_dev.h"):
        src = open(os.path.join(ROOT, "nyx_amd", "csrc", name)).read()
        assert "getenv" not in src and "environ" not in src and "hip_runtime" not in src, name
