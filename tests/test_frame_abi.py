"""CPU checks of the encounter boundary (include/nyx_hip_frame.h), the twin of tests/test_eclipse_abi.py: every declared function is
exported by the built library, the struct layout and the parameter codes match the ctypes mirror and `FrameParameter`, codes 0 .. 18
are `nyx_hip_state_param`'s, every refusal that can be told from the query alone is given before a device is touched - by both
flavours, the outputs left untouched -, the Python layer refuses what the device path refuses, and a C and a C++ program that include
only the new headers compile and link.  No compute calls (no GPU here).  What a query asks OF THE CONTEXT - a segment index beyond the
context's segments, the integration-frame swap refused with NYX_HIP_RC_UNSUPPORTED - needs a context, which needs a device: the rule
itself (`check_frame_context` of csrc/series_host.h, chained behind `check_frame_series` exactly as abi.cpp chains them) is run, with
every refusal and its message, by the stand-alone program of tests/test_frame_host_cxx.py (tests/cxx/frame_host_check.cpp), and
through the library on the GPU by tests/test_gpu_frame.py; here the source of abi.cpp is held to that chaining."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import nyx_amd as nx
from nyx_amd import _abi, frames
from nyx_amd.frames import FrameParameter as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nyx_hip_frame.h")


def _declared():
    return set(re.findall(r"^(?:int32_t|void|double|const char \*)\s*(nyx_hip_[a-z_0-9]+)\(", open(HEADER).read(), flags=re.M))


def _fields(header, struct):
    body = re.search(r"typedef struct %s \{(.*?)\} %s_t;" % (struct, struct), header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [re.sub(r"\[.*", "", n.strip()) for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]


def test_every_declared_frame_function_is_exported():
    lib = _abi.load_library()
    declared = _declared()
    assert declared == {"nyx_hip_traj_frame_values", "nyx_hip_traj_frame_values_device", "nyx_hip_frame_sizeof"}
    assert declared == set(_abi.FRAME_EXPORTS)
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in nyx_hip_frame.h but not exported"
        assert _abi.frame_entry(lib, name) is getattr(lib, name)
    # the entries stay out of the lists of the other headers (the Rust block is generated against EXPORTS)
    assert not declared & (set(_abi.EXPORTS) | set(_abi.REPORT_EXPORTS) | set(_abi.RIC_EXPORTS) | set(_abi.GROUNDTRACK_EXPORTS) | set(_abi.AER_EXPORTS)
                           | set(_abi.ECLIPSE_EXPORTS))
    # and nyx_hip.h does not know them: NYX_HIP_ABI_VERSION and its declaration list are unchanged
    main = open(os.path.join(ROOT, "include", "nyx_hip.h")).read()
    assert "nyx_hip_frame" not in main and "nyx_hip_traj_frame_values" not in main and "NYX_HIP_FRM" not in main


def test_an_older_library_gives_a_clear_error():
    class Old:   # a library built before the encounter report: no such symbol
        pass

    with pytest.raises(RuntimeError, match="has no nyx_hip_traj_frame_values.*rebuild"):
        _abi.frame_entry(Old())


def test_query_layout_and_constants_match_the_header():
    lib = _abi.load_library()
    header = open(HEADER).read()
    assert lib.nyx_hip_frame_sizeof(0) == C.sizeof(_abi.FrameQuery) == 4 + 4 + 32 + 3 * 8 + 4 + 16 + 16 + 4 + 8 == 112
    assert lib.nyx_hip_frame_sizeof(1) == _abi.FRAME_VERSION == int(re.search(r"#define NYX_HIP_FRAME_VERSION (\d+)", header).group(1))
    assert lib.nyx_hip_frame_sizeof(3) == _abi.MAX_FRAME_PARAMS == int(re.search(r"#define NYX_HIP_MAX_FRAME_PARAMS (\d+)", header).group(1)) == 8
    assert lib.nyx_hip_frame_sizeof(4) == -1 and lib.nyx_hip_frame_sizeof(-1) == -1
    # field order of the mirror = field order of the header
    assert _fields(header, "nyx_hip_frame_query") == [f for f, _ in _abi.FrameQuery._fields_]
    assert [getattr(_abi.FrameQuery, f).offset for f in ("n_params", "has_window", "param", "step_ns", "start_ns", "end_ns", "n_chain", "chain_segment",
                                                         "chain_sign", "_pad", "mu_km3_s2")] == [0, 4, 8, 40, 48, 56, 64, 68, 84, 100, 104]
    assert _abi.MAX_CHAIN == frames.MAX_CHAIN == int(re.search(r"#define NYX_HIP_MAX_CHAIN (\d+)", open(os.path.join(ROOT, "include", "nyx_hip.h")).read()).group(1))


def test_parameter_codes_match_the_header_and_cover_the_enum():
    lib = _abi.load_library()
    header = open(HEADER).read()
    enum = dict((k, int(v)) for k, v in re.findall(r"NYX_HIP_FRM_([A-Z_0-9]+) = (\d+)", header))
    count = enum.pop("COUNT")
    assert count == 25 == lib.nyx_hip_frame_sizeof(2) == _abi.FRAME_COUNT == len(F) == len(_abi.FRAME_PARAM)
    assert sorted(enum.values()) == list(range(19, 25))
    new = {name: code for name, code in _abi.FRAME_PARAM.items() if code >= 19}
    names = {"C3": "C3", "BdotT": "B_DOT_T", "BdotR": "B_DOT_R", "BAngle": "B_ANGLE", "BMagnitude": "B_MAGNITUDE", "VInfinity": "V_INFINITY"}
    assert {names[name]: code for name, code in new.items()} == enum == {"C3": 19, "B_DOT_T": 20, "B_DOT_R": 21, "B_ANGLE": 22, "B_MAGNITUDE": 23,
                                                                         "V_INFINITY": 24}
    assert {p.name: int(p) for p in F} == _abi.FRAME_PARAM
    # codes 0 .. 18 are enum nyx_hip_state_param's, in the header of the reports, in the mirror and in FrameParameter
    reports = open(os.path.join(ROOT, "include", "nyx_hip_reports.h")).read()
    sp = dict((k, int(v)) for k, v in re.findall(r"NYX_HIP_SP_([A-Z_]+) = (\d+)", reports))
    assert sp.pop("COUNT") == 19 == int(F.C3) and sorted(sp.values()) == list(range(19)) and len(_abi.STATE_PARAM) == 19
    assert {name: code for name, code in _abi.FRAME_PARAM.items() if code < 19} == _abi.STATE_PARAM
    for name, code in _abi.STATE_PARAM.items():
        assert int(F[name]) == code and frames.frame_param(nx.StateParameter[name]) is F[name]
    assert "BLTOF" not in _abi.FRAME_PARAM and "BLTOF" in header                  # no code, and the header says why
    assert '#include "nyx_hip_reports.h"' in header


def test_bad_queries_are_refused_before_any_device_is_touched():
    """Argument validation comes first: the same answer with and without a GPU, and never a clipped request."""
    lib = _abi.load_library()
    t = _abi.TrajBatch(2, 4)
    ct = t.as_c()
    values, length = np.zeros(8 * 4 * 2), np.zeros(2, dtype=np.int32)
    vp, lp = values.ctypes.data_as(_abi.c_double_p), length.ctypes.data_as(_abi.c_int32_p)
    fake_ctx = C.c_void_p(1)   # never dereferenced: every case below fails on the query alone
    nan, inf = float("nan"), float("inf")

    def query(n_params=1, param=int(F.BdotT), step=10**9, n_chain=3, mu=4902.8, segment=None, sign=None):
        q = _abi.FrameQuery()
        q.n_params, q.step_ns, q.n_chain, q.mu_km3_s2 = n_params, step, n_chain, mu
        for k in range(8):
            q.param[k] = param
        for k, (seg, sg) in enumerate([(2, 1), (1, -1), (0, -1), (3, 1)]):
            q.chain_segment[k], q.chain_sign[k] = seg, sg
        if segment:
            q.chain_segment[segment[0]] = segment[1]
        if sign:
            q.chain_sign[sign[0]] = sign[1]
        return q

    def refused(ctx, q, capacity, v, l, why, n=2):
        rc = lib.nyx_hip_traj_frame_values(ctx, C.byref(ct), n, C.byref(q) if q is not None else None, capacity, v, l)
        assert rc == _abi.RC_BAD_ARG and why in _abi.last_error(), (rc, _abi.last_error())
        rc = lib.nyx_hip_traj_frame_values_device(ctx, C.byref(ct), n, C.byref(q) if q is not None else None, capacity, v, l, None)
        assert rc == _abi.RC_BAD_ARG and why in _abi.last_error(), (rc, _abi.last_error())

    refused(None, query(), 4, vp, lp, "null ctx")
    refused(fake_ctx, None, 4, vp, lp, "traj_frame_values: null query")
    refused(fake_ctx, query(n_params=0), 4, vp, lp, "n_params = 0")
    refused(fake_ctx, query(n_params=9), 4, vp, lp, "n_params = 9")
    refused(fake_ctx, query(param=25), 4, vp, lp, "param[0] = 25 is not a nyx_hip_frame_param")
    refused(fake_ctx, query(param=-1), 4, vp, lp, "param[0] = -1")
    refused(fake_ctx, query(step=0), 4, vp, lp, "step_ns must be > 0")
    refused(fake_ctx, query(step=-5), 4, vp, lp, "step_ns must be > 0")
    refused(fake_ctx, query(), 0, vp, lp, "capacity")
    refused(fake_ctx, query(), 4, vp, lp, "negative n", n=-1)
    refused(fake_ctx, query(), 4, None, lp, "values and len arrays required")
    refused(fake_ctx, query(), 4, vp, None, "values and len arrays required")
    refused(fake_ctx, query(n_chain=-1), 4, vp, lp, "n_chain = -1, 0 .. 4")
    refused(fake_ctx, query(n_chain=5), 4, vp, lp, "n_chain = 5, 0 .. 4")
    refused(fake_ctx, query(segment=(1, -1)), 4, vp, lp, "chain_segment[1] = -1")
    refused(fake_ctx, query(sign=(2, 0)), 4, vp, lp, "chain_sign[2] = 0, +1 or -1")
    refused(fake_ctx, query(n_chain=4, sign=(3, 2)), 4, vp, lp, "chain_sign[3] = 2")
    for mu in (0.0, -1.0, nan, inf):
        refused(fake_ctx, query(mu=mu), 4, vp, lp, "mu_km3_s2 must be finite and > 0")
    assert (values == 0).all() and (length == 0).all()


def test_the_context_is_asked_behind_the_query_alone():
    """abi.cpp chains check_frame_series (never reads the context) and check_frame_context (its segments, no frame swap), in that
    order, in front of everything that touches a device - in both flavours."""
    src = open(os.path.join(ROOT, "nyx_amd", "csrc", "abi.cpp")).read()
    body = src[src.index("static Refusal check_frame("):]
    body = body[:body.index("\n}\n")]
    assert body.index("check_frame_series(ctx, traj, n, q, capacity, values, len)") < body.index("check_frame_context(*q, ctx->host_cfg.n_seg, ctx->swap_n_chain != 0)")
    for entry in ("nyx_hip_traj_frame_values_device", "nyx_hip_traj_frame_values"):
        fn = src[src.index(f'extern "C" int32_t {entry}('):]
        fn = fn[fn.index("{") + 1:fn.index("\n}\n")]
        assert fn.lstrip().startswith("if (Refusal r = check_frame(ctx, traj, n, q, capacity, values, len)) return refused(r);"), entry
    host = open(os.path.join(ROOT, "nyx_amd", "csrc", "series_host.h")).read()
    assert "NYX_HIP_RC_UNSUPPORTED" in host[host.index("inline Refusal check_frame_context("):host.index("inline Refusal check_ric_series(")]


def test_the_python_layer_refuses_what_the_device_path_refuses():
    class Ctx:   # no almanac: nothing to resolve a chain in
        compiled = None

    res = nx.Results([], "none", _traj_ctx=Ctx(), _traj_batch=_abi.TrajBatch(1, 2))
    moon = nx.Frame(nx.MOON, 4902.8)
    with pytest.raises(ValueError, match="a positive step"):
        res.frame_values(moon, [F.Rmag], 0)
    with pytest.raises(ValueError, match="at least one parameter"):
        res.frame_values(moon, [], 10**9)
    with pytest.raises(TypeError, match="not a"):
        res.frame_values(moon, [nx.StateParameter.Cr], 10**9)
    with pytest.raises(ValueError, match="does not know the almanac"):
        res.frame_values(moon, [F.Rmag], 10**9)
    with pytest.raises(ValueError, match="a window needs both"):
        res.frame_values(moon, [F.Rmag], 10**9, start_ns=5)
    series = nx.FrameSeries(moon, [F.BdotT], np.zeros((1, 0, 2)), np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int64), 10**9, np.ones(2, dtype=bool))
    with pytest.raises(ValueError, match="does not hold Rmag"):
        series.closest_approach()
    assert np.isnan(series.hyperbolic_fraction()).all()


def test_c_and_cxx_programs_compile_and_link(tmp_path):
    """include/nyx_hip_frame.h from C, include/nyx_hip_frame.hpp from C++: syntax alone, then against the built library (host only: the
    layout check runs, nothing is launched)."""
    _abi.load_library()
    inc = "-I" + os.path.join(ROOT, "include")
    link = ["-L" + os.path.join(ROOT, "nyx_amd"), "-lnyx_hip", "-Wl,-rpath," + os.path.join(ROOT, "nyx_amd")]
    c_src = tmp_path / "frm_check.c"
    c_src.write_text('#include "nyx_hip_frame.h"\n'
                     "int main(void) { nyx_hip_frame_query_t q; q.n_chain = 0; (void)q;\n"
                     "    return nyx_hip_frame_sizeof(0) == (int32_t)sizeof(nyx_hip_frame_query_t) && nyx_hip_frame_sizeof(2) == NYX_HIP_FRM_COUNT &&\n"
                     "           NYX_HIP_FRM_C3 == NYX_HIP_SP_PERIAPSIS_RADIUS + 1 && nyx_hip_frame_sizeof(1) == NYX_HIP_FRAME_VERSION ? 0 : 1; }\n")
    exe = str(tmp_path / "frm_check_c")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", inc, str(c_src), *link, "-o", exe], check=True)
    assert subprocess.run([exe]).returncode == 0
    src = tmp_path / "frm_check.cpp"
    src.write_text('#include "nyx_hip_frame.hpp"\n'
                   "nyx::FrameSeries encounter(nyx::GpuPropagator &p, nyx::TrajBatch &t, const nyx::FrameTarget &moon) {\n"
                   "    return nyx::traj_frame_values(p, t, moon, {NYX_HIP_SP_RMAG, NYX_HIP_SP_PERIAPSIS_RADIUS, NYX_HIP_FRM_B_DOT_T, NYX_HIP_FRM_B_DOT_R},\n"
                   "                                  60000000000LL, 1441);\n"
                   "}\n"
                   "int main() { return nyx_hip_frame_sizeof(0) == (int32_t)sizeof(nyx_hip_frame_query_t) && NYX_HIP_FRM_COUNT == 25 &&\n"
                   "             nyx_hip_frame_sizeof(3) == NYX_HIP_MAX_FRAME_PARAMS ? 0 : 1; }\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", inc, str(src)], check=True)
    exe = str(tmp_path / "frm_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", inc, str(src), *link, "-o", exe], check=True)
    assert subprocess.run([exe]).returncode == 0
