"""CPU checks of the report boundary (include/nyx_hip_reports.h): every declared function is exported by the built
library, the struct layout and the parameter codes match the ctypes mirror, and every orbit-derived member of
`StateParameter` has a code.  No compute calls (no GPU here); the declaration count of nyx_hip.h itself is held by
tests/test_abi.py."""
import ctypes as C
import os
import re

import pytest

import nyx_amd as nx
from nyx_amd import _abi
from nyx_amd.params import StateParameter as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nyx_hip_reports.h")

# Spacecraft-level members (constant over a run, filled on the host) and the two a ballistic state does not have
NOT_ORBIT = {P.Cr, P.Cd, P.DryMass, P.PropMass, P.TotalMass, P.Isp, P.Thrust}


def _declared():
    return set(re.findall(r"^(?:int32_t|void|double|const char \*)\s*(nyx_hip_[a-z_0-9]+)\(", open(HEADER).read(), flags=re.M))


def test_every_declared_report_function_is_exported():
    lib = _abi.load_library()
    declared = _declared()
    assert declared == {"nyx_hip_traj_values", "nyx_hip_traj_values_device", "nyx_hip_reports_sizeof"}
    assert declared == set(_abi.REPORT_EXPORTS)
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in nyx_hip_reports.h but not exported"
    # the report entries stay out of the list the Rust block is generated against
    assert not declared & set(_abi.EXPORTS)


def test_query_layout_and_constants_match_the_header():
    lib = _abi.load_library()
    header = open(HEADER).read()
    assert lib.nyx_hip_reports_sizeof(0) == C.sizeof(_abi.ValuesQuery) == 72
    assert lib.nyx_hip_reports_sizeof(1) == _abi.REPORTS_VERSION == int(re.search(r"#define NYX_HIP_REPORTS_VERSION (\d+)", header).group(1))
    assert lib.nyx_hip_reports_sizeof(3) == _abi.MAX_REPORT_PARAMS == int(re.search(r"#define NYX_HIP_MAX_REPORT_PARAMS (\d+)", header).group(1)) == 8
    assert lib.nyx_hip_reports_sizeof(99) == -1
    # field order of the mirror = field order of the header
    body = re.search(r"typedef struct nyx_hip_values_query \{(.*?)\} nyx_hip_values_query_t;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.sub(r"\[.*", "", n.strip()) for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert names == [f for f, _ in _abi.ValuesQuery._fields_]


def test_parameter_codes_match_the_header_and_cover_the_orbit_parameters():
    lib = _abi.load_library()
    header = open(HEADER).read()
    enum = dict((k, int(v)) for k, v in re.findall(r"NYX_HIP_SP_([A-Z_]+) = (\d+)", header))
    count = enum.pop("COUNT")
    assert count == len(enum) == 19 == lib.nyx_hip_reports_sizeof(2)
    assert sorted(enum.values()) == list(range(19))
    # header names are the StateParameter names in upper snake case
    assert {name.upper(): code for name, code in _abi.STATE_PARAM.items()} == {k.replace("_", ""): v for k, v in enum.items()}
    orbit = [p for p in P if p not in NOT_ORBIT]
    assert {p.name for p in orbit} == set(_abi.STATE_PARAM)
    for p in orbit:
        assert nx.report_param_code(p) == _abi.STATE_PARAM[p.name]
    for p in NOT_ORBIT:
        with pytest.raises(nx.StateError):
            nx.report_param_code(p)


def test_bad_queries_are_refused_before_any_device_is_touched():
    """Argument validation comes first: the same answer with and without a GPU, and never a clipped request."""
    lib = _abi.load_library()
    t = _abi.TrajBatch(2, 4)
    ct = t.as_c()
    import numpy as np
    values, length = np.zeros(8 * 4 * 2), np.zeros(2, dtype=np.int32)
    vp, lp = values.ctypes.data_as(_abi.c_double_p), length.ctypes.data_as(_abi.c_int32_p)
    fake_ctx = C.c_void_p(1)   # never dereferenced: every case below fails validation

    def query(n_params=1, param=0, step=10**9):
        q = _abi.ValuesQuery()
        q.n_params, q.step_ns = n_params, step
        for k in range(8):
            q.param[k] = param
        return q

    def refused(ctx, q, capacity, v, l, why):
        rc = lib.nyx_hip_traj_values(ctx, C.byref(ct), 2, C.byref(q) if q is not None else None, capacity, v, l)
        assert rc == _abi.RC_BAD_ARG and why in _abi.last_error(), (rc, _abi.last_error())
        rc = lib.nyx_hip_traj_values_device(ctx, C.byref(ct), 2, C.byref(q) if q is not None else None, capacity, v, l, None)
        assert rc == _abi.RC_BAD_ARG and why in _abi.last_error(), (rc, _abi.last_error())

    refused(None, query(), 4, vp, lp, "null ctx")
    refused(fake_ctx, None, 4, vp, lp, "null query")
    refused(fake_ctx, query(n_params=0), 4, vp, lp, "n_params = 0")
    refused(fake_ctx, query(n_params=9), 4, vp, lp, "n_params = 9")
    refused(fake_ctx, query(param=19), 4, vp, lp, "param[0] = 19")
    refused(fake_ctx, query(param=-1), 4, vp, lp, "param[0] = -1")
    refused(fake_ctx, query(step=0), 4, vp, lp, "step_ns must be > 0")
    refused(fake_ctx, query(), 0, vp, lp, "capacity")
    refused(fake_ctx, query(), 4, None, lp, "values and len arrays required")
    refused(fake_ctx, query(), 4, vp, None, "values and len arrays required")
    assert (values == 0).all() and (length == 0).all()


def test_cxx_wrapper_compiles_and_links(tmp_path):
    """include/nyx_hip_reports.hpp against the built library (host only: the layout check runs, nothing is launched)."""
    import subprocess
    _abi.load_library()
    src = tmp_path / "reports_check.cpp"
    src.write_text('#include "nyx_hip_reports.hpp"\n'
                   "nyx::ValueSeries sma_and_ecc(nyx::GpuPropagator &p, nyx::TrajBatch &t) {\n"
                   "    return nyx::traj_values(p, t, {NYX_HIP_SP_SEMI_MAJOR_AXIS, NYX_HIP_SP_ECCENTRICITY}, 60000000000LL, 1441);\n"
                   "}\n"
                   "int main() { return nyx_hip_reports_sizeof(0) == (int32_t)sizeof(nyx_hip_values_query_t) && NYX_HIP_SP_COUNT == 19 ? 0 : 1; }\n")
    exe = str(tmp_path / "reports_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + os.path.join(ROOT, "nyx_amd"),
                    "-lnyx_hip", "-Wl,-rpath," + os.path.join(ROOT, "nyx_amd"), "-o", exe], check=True)
    assert subprocess.run([exe]).returncode == 0
