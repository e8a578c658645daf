"""CPU: the host side of the station views (nyx_amd/csrc/series_host.h: `check_aer_series`; nyx_amd/csrc/aer_args.h:
`aer_station_consts`, `aer_param_needs`) as a stand-alone C++ program with its own `main` (tests/cxx/aer_host_check.cpp) - g++ only,
no HIP, no GPU - built with the address and undefined-behaviour sanitizers (their runtimes linked statically: the program does not
depend on which libraries the loader brings in first).  It runs `check_aer_series` over a table of cases (every
refusal of include/nyx_hip_aer.h and which check wins) and prints the constants of the stations given on its command line with
`%a`; those must equal `stations.station_consts` BIT FOR BIT: the kernel reads what the C function computes, the host definition
what the Python function computes, and the two are the same operations in the same order with the same C library."""
import os
import subprocess

import nyx_amd as nx
from nyx_amd import ephem
from nyx_amd.stations import station_consts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IAU_EARTH = nx.Frame(nx.EARTH, ephem.MU_EARTH, 6378.1363, nx.IAU_EARTH_ROTATION, 1.0 / 298.257)   # (the ellipsoid of the program's query)

# latitude, longitude, height, mask: the poles, longitude 0 / 180 / 243.205, a negative longitude, a height below the ellipsoid,
# and more than sixteen of them (two queries in the program)
STATIONS = [(90.0, 0.0, 0.0, 0.0), (-90.0, 0.0, 2.8, 10.0), (90.0, 243.205, 0.0, 5.0), (0.0, 0.0, 0.0, 0.0), (0.0, 180.0, 0.0, 0.0),
            (35.247164, 243.205, 1.07114904, 5.0), (40.427222, 4.250556, 0.834939, 5.0), (-35.398333, 148.981944, 0.691750, 7.5),
            (-33.1, -70.6, 0.7, 0.0), (1e-9, 359.999999999, -0.4, -3.0), (89.999999, 45.0, 0.0, 0.0), (-45.0, 725.0, 8.8, 90.0),
            (12.5, -179.9, 0.0, -90.0), (60.0, 60.0, 0.1, 1.0), (-60.0, 300.0, 0.2, 2.0), (30.0, 90.0, 0.3, 3.0), (-30.0, 270.0, 0.4, 4.0),
            (5.25, 52.8, 0.0, 5.0)]


def test_refusals_and_station_constants_bit_for_bit(tmp_path):
    exe = str(tmp_path / "aer_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                    "-static-libubsan", "-Wall",
                    "-Werror", os.path.join(ROOT, "tests", "cxx", "aer_host_check.cpp"), "-o", exe], check=True)
    args = [repr(float(v)) for st in STATIONS for v in st]
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "ok"
    got = [[float.fromhex(tok) for tok in ln.split()[1:]] for ln in lines if ln.startswith("consts")]
    assert len(got) == len(STATIONS) > 16
    for k, (lat, lon, h, mask) in enumerate(STATIONS):
        c = station_consts(nx.GroundStation(f"s{k}", lat, lon, h, IAU_EARTH, mask))
        want = [*c.r_km, *c.south, *c.east, *c.zenith, c.mask_deg]
        assert [v.hex() for v in got[k]] == [float(v).hex() for v in want], (k, STATIONS[k])


def test_the_station_constants_header_reads_no_environment_and_no_hip():
    src = open(os.path.join(ROOT, "nyx_amd", "csrc", "aer_args.h")).read()
    assert "getenv" not in src and "environ" not in src and "hip_runtime" not in src
