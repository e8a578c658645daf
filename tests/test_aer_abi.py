"""CPU checks of the station-view boundary (include/nyx_hip_aer.h), the twin of tests/test_groundtrack_abi.py: every declared
function is exported by the built library, the struct layouts and the parameter codes match the ctypes mirror, every member of
`AerParameter` has a code, every refusal of the header is given before a device is touched - by both flavours, the outputs left
untouched -, the Python layer refuses what the device path refuses, and the C++ wrapper compiles.  No compute calls (no GPU here)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import nyx_amd as nx
from nyx_amd import _abi, ephem
from nyx_amd.stations import AerParameter as A
from nyx_amd.stations import DEFAULT_PARAMS, check_stations

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nyx_hip_aer.h")
IAU_EARTH = nx.Frame(nx.EARTH, ephem.MU_EARTH, 6378.1363, nx.IAU_EARTH_ROTATION, 1.0 / 298.257)


def _declared():
    return set(re.findall(r"^(?:int32_t|void|double|const char \*)\s*(nyx_hip_[a-z_0-9]+)\(", open(HEADER).read(), flags=re.M))


def _fields(header, struct):
    body = re.search(r"typedef struct %s \{(.*?)\} %s_t;" % (struct, struct), header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [re.sub(r"\[.*", "", n.strip()) for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]


def test_every_declared_station_view_function_is_exported():
    lib = _abi.load_library()
    declared = _declared()
    assert declared == {"nyx_hip_traj_aer", "nyx_hip_traj_aer_device", "nyx_hip_aer_sizeof"}
    assert declared == set(_abi.AER_EXPORTS)
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in nyx_hip_aer.h but not exported"
        assert _abi.aer_entry(lib, name) is getattr(lib, name)
    # the entries stay out of the lists of the other headers (the Rust block is generated against EXPORTS)
    assert not declared & (set(_abi.EXPORTS) | set(_abi.REPORT_EXPORTS) | set(_abi.RIC_EXPORTS) | set(_abi.GROUNDTRACK_EXPORTS))


def test_an_older_library_gives_a_clear_error():
    class Old:   # a library built before the station views: no such symbol
        pass

    with pytest.raises(RuntimeError, match="has no nyx_hip_traj_aer.*rebuild"):
        _abi.aer_entry(Old())


def test_query_layout_and_constants_match_the_header():
    lib = _abi.load_library()
    header = open(HEADER).read()
    assert C.sizeof(_abi.Station) == 32
    assert lib.nyx_hip_aer_sizeof(0) == C.sizeof(_abi.AerQuery) == 88 + C.sizeof(_abi.Rotation) + 8 + 16 * 32 == 1408
    assert lib.nyx_hip_aer_sizeof(1) == _abi.AER_VERSION == int(re.search(r"#define NYX_HIP_AER_VERSION (\d+)", header).group(1))
    assert lib.nyx_hip_aer_sizeof(3) == _abi.MAX_AER_PARAMS == int(re.search(r"#define NYX_HIP_MAX_AER_PARAMS (\d+)", header).group(1)) == 8
    assert lib.nyx_hip_aer_sizeof(4) == _abi.MAX_STATIONS == int(re.search(r"#define NYX_HIP_MAX_STATIONS (\d+)", header).group(1)) == 16
    assert lib.nyx_hip_aer_sizeof(5) == -1 and lib.nyx_hip_aer_sizeof(-1) == -1
    # field order of the mirrors = field order of the header; the query opens with the fields of the ground-track query
    names = _fields(header, "nyx_hip_aer_query")
    assert names == [f for f, _ in _abi.AerQuery._fields_]
    assert names[:11] == [f for f, _ in _abi.GtQuery._fields_] and names[11:] == ["n_stations", "_pad2", "stations"]
    for f, _ in _abi.GtQuery._fields_:
        assert getattr(_abi.AerQuery, f).offset == getattr(_abi.GtQuery, f).offset, f
    assert [getattr(_abi.AerQuery, f).offset for f in ("n_stations", "stations")] == [888, 896]
    assert _fields(header, "nyx_hip_station") == [f for f, _ in _abi.Station._fields_] == ["latitude_deg", "longitude_deg", "height_km", "elevation_mask_deg"]


def test_parameter_codes_match_the_header_and_cover_the_enum():
    lib = _abi.load_library()
    header = open(HEADER).read()
    enum = dict((k, int(v)) for k, v in re.findall(r"NYX_HIP_AER_([A-Z_]+) = (\d+)", header))
    count = enum.pop("COUNT")
    assert count == len(enum) == 9 == lib.nyx_hip_aer_sizeof(2)
    assert sorted(enum.values()) == list(range(9))
    assert {re.sub(r"(?<!^)(?=[A-Z])", "_", name).upper(): code for name, code in _abi.AER_PARAM.items()} == enum
    assert {p.name for p in A} == set(_abi.AER_PARAM)
    for p in A:
        assert nx.aer_param_code(p) == _abi.AER_PARAM[p.name]
    assert [nx.aer_param_code(p) for p in DEFAULT_PARAMS] == [0, 1, 2, 3]
    # a ground-track parameter is not a station-view parameter
    with pytest.raises(TypeError):
        nx.aer_param_code(nx.GroundTrackParameter.Latitude)


def test_bad_queries_are_refused_before_any_device_is_touched():
    """Argument validation comes first: the same answer with and without a GPU, and never a clipped request."""
    lib = _abi.load_library()
    t = _abi.TrajBatch(2, 4)
    ct = t.as_c()
    values, length = np.zeros(16 * 8 * 4 * 2), np.zeros(2, dtype=np.int32)
    vp, lp = values.ctypes.data_as(_abi.c_double_p), length.ctypes.data_as(_abi.c_int32_p)
    fake_ctx = C.c_void_p(1)   # never dereferenced: every case below fails validation
    nan, inf = float("nan"), float("inf")

    def query(n_params=1, param=_abi.AER_PARAM["Range"], step=10**9, kind=_abi.ROT_IAU, terms=0, radius=6378.1363, flattening=1.0 / 298.257,
              n_stations=2, station=None, at=1):
        q = _abi.AerQuery()
        q.n_params, q.step_ns, q.has_frame = n_params, step, 1
        for k in range(8):
            q.param[k] = param
        q.frame.kind, q.frame.n_nut_prec = kind, terms
        q.frame_eq_radius_km, q.frame_flattening = radius, flattening
        q.n_stations = n_stations
        for k in range(16):
            q.stations[k].latitude_deg, q.stations[k].longitude_deg, q.stations[k].height_km, q.stations[k].elevation_mask_deg = 40.0, 4.0, 0.8, 5.0
        for f, v in (station or {}).items():
            setattr(q.stations[at], f, v)
        return q

    def refused(ctx, q, capacity, v, l, why, n=2):
        rc = lib.nyx_hip_traj_aer(ctx, C.byref(ct), n, C.byref(q) if q is not None else None, capacity, v, l)
        assert rc == _abi.RC_BAD_ARG and why in _abi.last_error(), (rc, _abi.last_error())
        rc = lib.nyx_hip_traj_aer_device(ctx, C.byref(ct), n, C.byref(q) if q is not None else None, capacity, v, l, None)
        assert rc == _abi.RC_BAD_ARG and why in _abi.last_error(), (rc, _abi.last_error())

    refused(None, query(), 4, vp, lp, "null ctx")
    refused(fake_ctx, None, 4, vp, lp, "null query")
    refused(fake_ctx, query(n_params=0), 4, vp, lp, "n_params = 0")
    refused(fake_ctx, query(n_params=9), 4, vp, lp, "n_params = 9")
    refused(fake_ctx, query(param=9), 4, vp, lp, "param[0] = 9")
    refused(fake_ctx, query(param=-1), 4, vp, lp, "param[0] = -1")
    refused(fake_ctx, query(step=0), 4, vp, lp, "step_ns must be > 0")
    refused(fake_ctx, query(step=-5), 4, vp, lp, "step_ns must be > 0")
    refused(fake_ctx, query(), 0, vp, lp, "capacity")
    refused(fake_ctx, query(), 4, vp, lp, "negative n", n=-1)
    refused(fake_ctx, query(), 4, None, lp, "values and len arrays required")
    refused(fake_ctx, query(), 4, vp, None, "values and len arrays required")
    refused(fake_ctx, query(n_stations=0), 4, vp, lp, "n_stations = 0")
    refused(fake_ctx, query(n_stations=-1), 4, vp, lp, "n_stations = -1")
    refused(fake_ctx, query(n_stations=17), 4, vp, lp, "n_stations = 17")
    refused(fake_ctx, query(station={"latitude_deg": 90.000001}), 4, vp, lp, "stations[1].latitude_deg")
    refused(fake_ctx, query(station={"latitude_deg": -91.0}, at=0), 4, vp, lp, "stations[0].latitude_deg")
    refused(fake_ctx, query(station={"latitude_deg": nan}), 4, vp, lp, "stations[1].latitude_deg")
    refused(fake_ctx, query(station={"longitude_deg": inf}), 4, vp, lp, "stations[1].longitude_deg")
    refused(fake_ctx, query(station={"longitude_deg": nan}, at=0), 4, vp, lp, "stations[0].longitude_deg")
    refused(fake_ctx, query(station={"height_km": -inf}), 4, vp, lp, "stations[1].height_km")
    refused(fake_ctx, query(station={"height_km": nan}, n_stations=16, at=15), 4, vp, lp, "stations[15].height_km")
    refused(fake_ctx, query(station={"elevation_mask_deg": 90.5}), 4, vp, lp, "stations[1].elevation_mask_deg")
    refused(fake_ctx, query(station={"elevation_mask_deg": -91.0}), 4, vp, lp, "stations[1].elevation_mask_deg")
    refused(fake_ctx, query(station={"elevation_mask_deg": nan}), 4, vp, lp, "stations[1].elevation_mask_deg")
    refused(fake_ctx, query(kind=_abi.ROT_EULER_CHEBY), 4, vp, lp, "NYX_HIP_ROT_IAU")
    refused(fake_ctx, query(terms=-1), 4, vp, lp, "n_nut_prec = -1")
    refused(fake_ctx, query(terms=_abi.MAX_NUT_PREC + 1), 4, vp, lp, "n_nut_prec = 17")
    refused(fake_ctx, query(radius=0.0), 4, vp, lp, "frame_eq_radius_km must be > 0")      # (always needed: whatever the parameter)
    refused(fake_ctx, query(radius=-1.0), 4, vp, lp, "frame_eq_radius_km must be > 0")
    refused(fake_ctx, query(radius=nan), 4, vp, lp, "frame_eq_radius_km must be > 0")
    refused(fake_ctx, query(flattening=-1e-3), 4, vp, lp, "frame_flattening")
    refused(fake_ctx, query(flattening=1.0), 4, vp, lp, "frame_flattening")
    refused(fake_ctx, query(flattening=nan), 4, vp, lp, "frame_flattening")
    assert (values == 0).all() and (length == 0).all()


def test_the_python_layer_refuses_what_the_device_path_refuses():
    st = lambda **kw: nx.GroundStation(**{**dict(name="s", latitude_deg=40.0, longitude_deg=4.0, height_km=0.8, frame=IAU_EARTH), **kw})
    assert check_stations([st(), st(latitude_deg=-90.0, elevation_mask_deg=90.0)], nx.EARTH) is IAU_EARTH
    with pytest.raises(ValueError, match="at least one station"):
        check_stations([])
    for bad in (dict(latitude_deg=90.5), dict(latitude_deg=float("nan")), dict(longitude_deg=float("inf")), dict(height_km=float("nan")),
                dict(elevation_mask_deg=-91.0)):
        with pytest.raises(ValueError, match=r"stations\[1\]"):
            check_stations([st(), st(**bad)])
    with pytest.raises(TypeError):
        check_stations([st(), (40.0, 4.0, 0.8)])
    other = nx.Frame(nx.EARTH, ephem.MU_EARTH, 6378.1363, nx.IAU_EARTH_ROTATION, 0.0)
    with pytest.raises(ValueError, match="share one frame"):
        check_stations([st(), st(frame=other)])
    with pytest.raises(NotImplementedError, match="same centre"):
        check_stations([st()], central_naif_id=nx.MOON)
    with pytest.raises(ValueError, match="equatorial radius"):
        check_stations([st(frame=nx.Frame(nx.EARTH, ephem.MU_EARTH, 0.0, nx.IAU_EARTH_ROTATION, 0.0))])
    with pytest.raises(ValueError, match="flattening"):
        check_stations([st(frame=nx.Frame(nx.EARTH, ephem.MU_EARTH, 6378.1363, nx.IAU_EARTH_ROTATION, 1.0))])


def test_cxx_wrapper_compiles_and_links(tmp_path):
    """include/nyx_hip_aer.hpp: syntax alone, then against the built library (host only: the layout check runs, nothing is
    launched)."""
    _abi.load_library()
    src = tmp_path / "aer_check.cpp"
    src.write_text('#include "nyx_hip_aer.hpp"\n'
                   "nyx::AerSeries views(nyx::GpuPropagator &p, nyx::TrajBatch &t, const nyx::StationFrame &f) {\n"
                   "    return nyx::traj_aer(p, t, f, {{40.427222, 4.250556, 0.834939, 5.0}}, {NYX_HIP_AER_AZIMUTH, NYX_HIP_AER_ELEVATION,\n"
                   "                         NYX_HIP_AER_RANGE, NYX_HIP_AER_RANGE_RATE}, 60000000000LL, 1441);\n"
                   "}\n"
                   "int main() { return nyx_hip_aer_sizeof(0) == (int32_t)sizeof(nyx_hip_aer_query_t) && NYX_HIP_AER_COUNT == 9 &&\n"
                   "             nyx_hip_aer_sizeof(4) == NYX_HIP_MAX_STATIONS ? 0 : 1; }\n")
    inc = "-I" + os.path.join(ROOT, "include")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", inc, str(src)], check=True)
    exe = str(tmp_path / "aer_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", inc, str(src), "-L" + os.path.join(ROOT, "nyx_amd"),
                    "-lnyx_hip", "-Wl,-rpath," + os.path.join(ROOT, "nyx_amd"), "-o", exe], check=True)
    assert subprocess.run([exe]).returncode == 0
