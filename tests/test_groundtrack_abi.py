"""CPU checks of the ground-track boundary (include/nyx_hip_groundtrack.h): every declared function is exported by the built
library, the struct layout and the parameter codes match the ctypes mirror, every member of `GroundTrackParameter` has a
code, every refusal of the header is given before a device is touched, and the C++ wrapper compiles.  No compute calls
(no GPU here); nyx_hip.h and nyx_hip_reports.h keep their own tests."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import nyx_amd as nx
from nyx_amd import _abi
from nyx_amd.groundtrack import GroundTrackParameter as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nyx_hip_groundtrack.h")


def _declared():
    return set(re.findall(r"^(?:int32_t|void|double|const char \*)\s*(nyx_hip_[a-z_0-9]+)\(", open(HEADER).read(), flags=re.M))


def test_every_declared_ground_track_function_is_exported():
    lib = _abi.load_library()
    declared = _declared()
    assert declared == {"nyx_hip_traj_ground_track", "nyx_hip_traj_ground_track_device", "nyx_hip_groundtrack_sizeof"}
    assert declared == set(_abi.GROUNDTRACK_EXPORTS)
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in nyx_hip_groundtrack.h but not exported"
        assert _abi.ground_track_entry(lib, name) is getattr(lib, name)
    # the entries stay out of the lists of the other headers (the Rust block is generated against EXPORTS)
    assert not declared & (set(_abi.EXPORTS) | set(_abi.REPORT_EXPORTS) | set(_abi.RIC_EXPORTS))


def test_an_older_library_gives_a_clear_error():
    class Old:   # a library built before the ground tracks: no such symbol
        pass

    with pytest.raises(RuntimeError, match="has no nyx_hip_traj_ground_track.*rebuild"):
        _abi.ground_track_entry(Old())


def test_query_layout_and_constants_match_the_header():
    lib = _abi.load_library()
    header = open(HEADER).read()
    assert lib.nyx_hip_groundtrack_sizeof(0) == C.sizeof(_abi.GtQuery) == 88 + C.sizeof(_abi.Rotation) == 888
    assert lib.nyx_hip_groundtrack_sizeof(1) == _abi.GROUNDTRACK_VERSION == int(re.search(r"#define NYX_HIP_GROUNDTRACK_VERSION (\d+)", header).group(1))
    assert lib.nyx_hip_groundtrack_sizeof(3) == _abi.MAX_GT_PARAMS == int(re.search(r"#define NYX_HIP_MAX_GT_PARAMS (\d+)", header).group(1)) == 8
    assert lib.nyx_hip_groundtrack_sizeof(99) == -1
    # field order of the mirror = field order of the header
    body = re.search(r"typedef struct nyx_hip_gt_query \{(.*?)\} nyx_hip_gt_query_t;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.sub(r"\[.*", "", n.strip()) for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert names == [f for f, _ in _abi.GtQuery._fields_]
    assert names == ["n_params", "param", "has_window", "step_ns", "start_ns", "end_ns", "has_frame", "_pad", "frame_eq_radius_km",
                     "frame_flattening", "frame"]
    assert [getattr(_abi.GtQuery, f).offset for f in ("param", "has_window", "step_ns", "has_frame", "frame_eq_radius_km", "frame")] == [4, 36, 40, 64, 72, 88]


def test_parameter_codes_match_the_header_and_cover_the_enum():
    lib = _abi.load_library()
    header = open(HEADER).read()
    enum = dict((k, int(v)) for k, v in re.findall(r"NYX_HIP_GT_([A-Z_]+) = (\d+)", header))
    count = enum.pop("COUNT")
    assert count == len(enum) == 12 == lib.nyx_hip_groundtrack_sizeof(2)
    assert sorted(enum.values()) == list(range(12))
    assert {name.upper(): code for name, code in _abi.GT_PARAM.items()} == enum
    assert {p.name for p in G} == set(_abi.GT_PARAM)
    for p in G:
        assert nx.gt_param_code(p) == _abi.GT_PARAM[p.name]
    # a StateParameter of the same name is not a ground-track parameter: the orbit reports keep their enum
    with pytest.raises(TypeError):
        nx.gt_param_code(nx.StateParameter.Rmag)
    assert not hasattr(nx.StateParameter, "Latitude") and len(_abi.STATE_PARAM) == 19


def test_bad_queries_are_refused_before_any_device_is_touched():
    """Argument validation comes first: the same answer with and without a GPU, and never a clipped request."""
    lib = _abi.load_library()
    t = _abi.TrajBatch(2, 4)
    ct = t.as_c()
    values, length = np.zeros(8 * 4 * 2), np.zeros(2, dtype=np.int32)
    vp, lp = values.ctypes.data_as(_abi.c_double_p), length.ctypes.data_as(_abi.c_int32_p)
    fake_ctx = C.c_void_p(1)   # never dereferenced: every case below fails validation

    def query(n_params=1, param=_abi.GT_PARAM["X"], step=10**9, kind=_abi.ROT_IAU, terms=0, radius=6378.1363, flattening=1.0 / 298.257):
        q = _abi.GtQuery()
        q.n_params, q.step_ns, q.has_frame = n_params, step, 1
        for k in range(8):
            q.param[k] = param
        q.frame.kind, q.frame.n_nut_prec = kind, terms
        q.frame_eq_radius_km, q.frame_flattening = radius, flattening
        return q

    def refused(ctx, q, capacity, v, l, why, n=2):
        rc = lib.nyx_hip_traj_ground_track(ctx, C.byref(ct), n, C.byref(q) if q is not None else None, capacity, v, l)
        assert rc == _abi.RC_BAD_ARG and why in _abi.last_error(), (rc, _abi.last_error())
        rc = lib.nyx_hip_traj_ground_track_device(ctx, C.byref(ct), n, C.byref(q) if q is not None else None, capacity, v, l, None)
        assert rc == _abi.RC_BAD_ARG and why in _abi.last_error(), (rc, _abi.last_error())

    lat = _abi.GT_PARAM["Latitude"]
    refused(None, query(), 4, vp, lp, "null ctx")
    refused(fake_ctx, None, 4, vp, lp, "null query")
    refused(fake_ctx, query(n_params=0), 4, vp, lp, "n_params = 0")
    refused(fake_ctx, query(n_params=9), 4, vp, lp, "n_params = 9")
    refused(fake_ctx, query(param=12), 4, vp, lp, "param[0] = 12")
    refused(fake_ctx, query(param=-1), 4, vp, lp, "param[0] = -1")
    refused(fake_ctx, query(step=0), 4, vp, lp, "step_ns must be > 0")
    refused(fake_ctx, query(step=-5), 4, vp, lp, "step_ns must be > 0")
    refused(fake_ctx, query(), 0, vp, lp, "capacity")
    refused(fake_ctx, query(), 4, vp, lp, "negative n", n=-1)
    refused(fake_ctx, query(), 4, None, lp, "values and len arrays required")
    refused(fake_ctx, query(), 4, vp, None, "values and len arrays required")
    refused(fake_ctx, query(kind=_abi.ROT_EULER_CHEBY), 4, vp, lp, "NYX_HIP_ROT_IAU")
    refused(fake_ctx, query(terms=-1), 4, vp, lp, "n_nut_prec = -1")
    refused(fake_ctx, query(terms=_abi.MAX_NUT_PREC + 1), 4, vp, lp, "n_nut_prec = 17")
    refused(fake_ctx, query(param=lat, radius=0.0), 4, vp, lp, "frame_eq_radius_km > 0")
    refused(fake_ctx, query(param=_abi.GT_PARAM["Height"], radius=-1.0), 4, vp, lp, "frame_eq_radius_km > 0")
    refused(fake_ctx, query(param=lat, radius=float("nan")), 4, vp, lp, "frame_eq_radius_km > 0")
    refused(fake_ctx, query(flattening=-1e-3), 4, vp, lp, "frame_flattening")
    refused(fake_ctx, query(flattening=1.0), 4, vp, lp, "frame_flattening")
    refused(fake_ctx, query(flattening=float("nan")), 4, vp, lp, "frame_flattening")
    assert (values == 0).all() and (length == 0).all()


def test_cxx_wrapper_compiles_and_links(tmp_path):
    """include/nyx_hip_groundtrack.hpp: syntax alone, then against the built library (host only: the layout check runs,
    nothing is launched)."""
    _abi.load_library()
    src = tmp_path / "groundtrack_check.cpp"
    src.write_text('#include "nyx_hip_groundtrack.hpp"\n'
                   "nyx::GroundTrackSeries track(nyx::GpuPropagator &p, nyx::TrajBatch &t, const nyx::GroundFrame &f) {\n"
                   "    return nyx::traj_ground_track(p, t, f, {NYX_HIP_GT_LATITUDE, NYX_HIP_GT_LONGITUDE, NYX_HIP_GT_HEIGHT, NYX_HIP_GT_RMAG}, 60000000000LL, 1441);\n"
                   "}\n"
                   "int main() { return nyx_hip_groundtrack_sizeof(0) == (int32_t)sizeof(nyx_hip_gt_query_t) && NYX_HIP_GT_COUNT == 12 ? 0 : 1; }\n")
    inc = "-I" + os.path.join(ROOT, "include")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", inc, str(src)], check=True)
    exe = str(tmp_path / "groundtrack_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", inc, str(src), "-L" + os.path.join(ROOT, "nyx_amd"),
                    "-lnyx_hip", "-Wl,-rpath," + os.path.join(ROOT, "nyx_amd"), "-o", exe], check=True)
    assert subprocess.run([exe]).returncode == 0
