"""CPU checks of the Lambert boundary (include/nyx_hip_lambert.h), the twin of tests/test_frame_abi.py: every declared function is
exported by the built library, the struct layouts and the codes match the ctypes mirrors and the enums of nyx_amd/lambert.py, every
refusal that can be told from the arguments alone is given before a device is touched - by both flavours of both entries, the outputs
left untouched, in the order the header lists them -, and a C and a C++ program that include only the new headers compile and link.
No compute calls (no GPU here).  What a grid asks OF THE CONTEXT - a segment index beyond the context's, the integration-frame swap -
needs a context, which needs a device: tests/test_gpu_lambert.py; here the source of abi.cpp is held to the chaining."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from nyx_amd import _abi, lambert

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nyx_hip_lambert.h")


def _fields(header, struct):
    body = re.search(r"typedef struct %s \{(.*?)\} %s_t;" % (struct, struct), header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [re.sub(r"\[.*", "", n.strip()) for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]


def test_every_declared_lambert_function_is_exported():
    lib = _abi.load_library()
    declared = set(re.findall(r"^(?:int32_t|void|double|const char \*)\s*(nyx_hip_[a-z_0-9]+)\(", open(HEADER).read(), flags=re.M))
    assert declared == {"nyx_hip_lambert_batch", "nyx_hip_lambert_batch_device", "nyx_hip_lambert_grid", "nyx_hip_lambert_grid_device",
                        "nyx_hip_lambert_sizeof"} == set(_abi.LAMBERT_EXPORTS)
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in nyx_hip_lambert.h but not exported"
        assert _abi.lambert_entry(lib, name) is getattr(lib, name)
    others = (_abi.EXPORTS, _abi.REPORT_EXPORTS, _abi.RIC_EXPORTS, _abi.GROUNDTRACK_EXPORTS, _abi.AER_EXPORTS, _abi.ECLIPSE_EXPORTS, _abi.FRAME_EXPORTS,
              _abi.LINK_EXPORTS, _abi.STATS_EXPORTS)
    assert not any(declared & set(o) for o in others)
    # nyx_hip.h does not know them: NYX_HIP_ABI_VERSION and its declaration list are unchanged
    main = open(os.path.join(ROOT, "include", "nyx_hip.h")).read()
    assert "lambert" not in main and "NYX_HIP_LMB" not in main

    class Old:   # a library built before the Lambert transfers: no such symbol
        pass

    with pytest.raises(RuntimeError, match="has no nyx_hip_lambert_grid.*rebuild"):
        _abi.lambert_entry(Old())


def test_layouts_and_codes_match_the_header():
    lib = _abi.load_library()
    header = open(HEADER).read()
    assert lib.nyx_hip_lambert_sizeof(0) == C.sizeof(_abi.LambertQuery) == 4 + 32 + 5 * 4 + 8 == 64
    assert lib.nyx_hip_lambert_sizeof(5) == C.sizeof(_abi.LambertChain) == 4 + 16 + 16 + 4 == 40
    assert lib.nyx_hip_lambert_sizeof(4) == C.sizeof(_abi.LambertGridQuery) == 64 + 3 * 40 + 8 + 8 * 8 + 8 == 264
    assert lib.nyx_hip_lambert_sizeof(1) == _abi.LAMBERT_VERSION == int(re.search(r"#define NYX_HIP_LAMBERT_VERSION (\d+)", header).group(1))
    assert lib.nyx_hip_lambert_sizeof(3) == _abi.MAX_LAMBERT_PARAMS == lambert.MAX_PARAMS == int(re.search(r"#define NYX_HIP_MAX_LAMBERT_PARAMS (\d+)", header).group(1)) == 8
    assert lib.nyx_hip_lambert_sizeof(6) == -1 and lib.nyx_hip_lambert_sizeof(-1) == -1
    for struct, mirror in (("nyx_hip_lambert_query", _abi.LambertQuery), ("nyx_hip_lambert_chain", _abi.LambertChain), ("nyx_hip_lambert_grid_query", _abi.LambertGridQuery)):
        assert _fields(header, struct) == [f for f, _ in mirror._fields_], struct
    assert [getattr(_abi.LambertQuery, f).offset for f in ("n_params", "param", "way", "n_revs", "high_path", "max_iter", "_pad", "tol")] == [0, 4, 36, 40, 44, 48, 52, 56]
    assert [getattr(_abi.LambertGridQuery, f).offset for f in ("solve", "dep", "arr", "centre", "has_tof", "n_dep", "n_arr", "dep0_ns", "dep_step_ns", "arr0_ns",
                                                               "arr_step_ns", "tof0_ns", "tof_step_ns", "mu_km3_s2")] == [0, 64, 104, 144, 184, 192, 200, 208, 216, 224, 232, 240, 248, 256]
    # the enums are pinned: never renumbered
    params = dict((k, int(v)) for k, v in re.findall(r"NYX_HIP_LMB_([A-Z_0-9]+) = (\d+)", header))
    assert [params[k] for k in ("V1X", "V1Y", "V1Z", "V2X", "V2Y", "V2Z", "X", "ITERATIONS", "TOF_S", "TRANSFER_ANGLE_DEG", "C3", "VINF_DEP", "DLA_DEG", "RLA_DEG",
                                "VINF_ARR", "DV_TOTAL", "COUNT")] == list(range(17))
    assert lib.nyx_hip_lambert_sizeof(2) == 16 == _abi.LAMBERT_COUNT == len(lambert.LambertParameter) == lambert.N_VALUES
    assert {p.name: int(p) for p in lambert.LambertParameter} == _abi.LAMBERT_PARAM
    assert [params[k] for k in ("AUTO", "SHORT", "LONG", "WAY_COUNT")] == [0, 1, 2, 3] and {w.name: int(w) for w in lambert.TransferKind} == _abi.LAMBERT_WAY
    assert [params[k] for k in ("OK", "BAD_INPUT", "DEGENERATE", "NOT_FEASIBLE", "TOO_CLOSE", "MAX_ITER_HIT", "EPHEM_RANGE")] == list(range(7))
    assert {s.name: int(s) for s in lambert.LambertStatus} == _abi.LAMBERT_STATUS
    assert [int(re.search(r"#define NYX_HIP_LMB_%s (\S+)" % k, header).group(1)) for k in ("SERIES_MAX", "MAX_REVS", "MAX_ITER")] == [
        lambert.SERIES_MAX, lambert.MAX_REVS, lambert.MAX_ITER_MOST] == [64, 255, 1000]
    assert (lambert.TOL_MIN, lambert.TOL_MAX, lambert.DEFAULT_TOL, lambert.DEFAULT_MAX_ITER) == (1e-13, 1e-2, 1e-4, 1000)


def solver(q, **kw):
    q.n_params, q.way, q.n_revs, q.high_path, q.max_iter, q.tol = 1, 0, 0, 0, 1000, 1e-4
    q.param[0] = int(lambert.LambertParameter.C3)
    for k, v in kw.items():
        if k == "param":
            q.param[v[0]] = v[1]
        else:
            setattr(q, k, v)


SOLVER_REFUSALS = [(dict(n_params=0), "n_params = 0, 1 .. 8"), (dict(n_params=9), "n_params = 9"), (dict(param=(0, 16)), "param[0] = 16 is not a nyx_hip_lambert_param"),
                   (dict(param=(0, -1)), "param[0] = -1"), (dict(n_params=2, param=(1, 99)), "param[1] = 99"), (dict(way=3), "way = 3 is not a nyx_hip_lambert_way"),
                   (dict(way=-1), "way = -1"), (dict(n_revs=-1), "n_revs = -1, 0 .. 255"), (dict(n_revs=256), "n_revs = 256"), (dict(high_path=2), "high_path = 2, 0 or 1"),
                   (dict(tol=1e-14), "tol = 1e-14, 1e-13 .. 1e-2"), (dict(tol=0.1), "tol = 0.1"), (dict(tol=float("nan")), "tol = nan"),
                   (dict(max_iter=0), "max_iter = 0, 1 .. 1000"), (dict(max_iter=1001), "max_iter = 1001"),
                   # which check wins: the first of the header's list
                   (dict(n_params=0, way=7, tol=1.0), "n_params = 0"), (dict(way=7, n_revs=999, tol=1.0), "way = 7"), (dict(n_revs=999, max_iter=0), "n_revs = 999"),
                   (dict(tol=1.0, max_iter=0), "tol = 1")]


def test_bad_batches_are_refused_before_any_device_is_touched():
    lib = _abi.load_library()
    rv, tof, values, status = np.zeros(12), np.ones(2), np.zeros(16), np.zeros(2, dtype=np.int32)
    dp = lambda a: a.ctypes.data_as(_abi.c_double_p)   # noqa: E731
    sp = status.ctypes.data_as(_abi.c_int32_p)
    fake_ctx = C.c_void_p(1)   # never dereferenced: every case below fails on the arguments alone

    def refused(why, ctx=fake_ctx, q="default", mu=398600.4, n=2, rv1=dp(rv), rv2=dp(rv), t=dp(tof), v=dp(values), s=sp, **kw):
        if q == "default":
            q = _abi.LambertQuery()
            solver(q, **kw)
        ref = C.byref(q) if q is not None else None
        for rc in (lib.nyx_hip_lambert_batch(ctx, rv1, rv2, t, n, mu, ref, v, s), lib.nyx_hip_lambert_batch_device(ctx, rv1, rv2, t, n, mu, ref, v, s, None)):
            assert rc == _abi.RC_BAD_ARG and why in _abi.last_error(), (why, rc, _abi.last_error())

    refused("null ctx", ctx=None)
    refused("lambert_batch: null query", q=None)
    for kw, why in SOLVER_REFUSALS:
        refused("lambert_batch: " + why, **kw)
    for mu in (0.0, -1.0, float("nan"), float("inf")):
        refused("lambert_batch: mu_km3_s2 must be finite and > 0", mu=mu)
    refused("lambert_batch: max_iter = 0", max_iter=0, mu=0.0, n=-1)     # the solver's settings before mu, mu before n
    refused("mu_km3_s2", mu=0.0, n=-1)
    refused("negative n", n=-1, rv1=None)
    refused("rv1, rv2 and tof_s arrays required", rv1=None, v=None)
    refused("rv1, rv2 and tof_s arrays required", rv2=None)
    refused("rv1, rv2 and tof_s arrays required", t=None)
    refused("values and status arrays required", v=None)
    refused("values and status arrays required", s=None)
    assert (values == 0).all() and (status == 0).all()
    # n = 0 is legal and launches nothing (no device is touched: the context is never dereferenced)
    q = _abi.LambertQuery()
    solver(q)
    assert lib.nyx_hip_lambert_batch(fake_ctx, dp(rv), dp(rv), dp(tof), 0, 398600.4, C.byref(q), dp(values), sp) == 0
    assert lib.nyx_hip_lambert_batch_device(fake_ctx, dp(rv), dp(rv), dp(tof), 0, 398600.4, C.byref(q), dp(values), sp, None) == 0


def test_bad_grids_are_refused_before_any_device_is_touched():
    lib = _abi.load_library()
    values, status = np.zeros(8 * 6), np.zeros(6, dtype=np.int32)
    vp, sp = values.ctypes.data_as(_abi.c_double_p), status.ctypes.data_as(_abi.c_int32_p)
    fake_ctx = C.c_void_p(1)

    def grid(**kw):
        q = _abi.LambertGridQuery()
        solver(q.solve, **{k: kw.pop(k) for k in list(kw) if k in ("n_params", "param", "way", "n_revs", "high_path", "tol", "max_iter")})
        q.n_dep, q.n_arr, q.dep_step_ns, q.arr_step_ns, q.tof_step_ns, q.mu_km3_s2 = 2, 3, 10**9, 10**9, 10**9, 1.327e11
        for dst, chain in ((q.dep, [(2, 1), (1, -1)]), (q.arr, [(3, 1), (1, -1)]), (q.centre, [(1, -1)])):
            dst.n_chain = len(chain)
            for k, (seg, sign) in enumerate(chain):
                dst.chain_segment[k], dst.chain_sign[k] = seg, sign
        for k, v in kw.items():
            if k in ("dep", "arr", "centre"):
                dst = getattr(q, k)
                for f, val in v.items():
                    if f == "n_chain":
                        dst.n_chain = val
                    else:
                        getattr(dst, f)[val[0]] = val[1]
            else:
                setattr(q, k, v)
        return q

    def refused(why, ctx=fake_ctx, q="default", v=vp, s=sp, **kw):
        q = grid(**kw) if q == "default" else q
        ref = C.byref(q) if q is not None else None
        for rc in (lib.nyx_hip_lambert_grid(ctx, ref, v, s), lib.nyx_hip_lambert_grid_device(ctx, ref, v, s, None)):
            assert rc == _abi.RC_BAD_ARG and why in _abi.last_error(), (why, rc, _abi.last_error())

    refused("null ctx", ctx=None)
    refused("lambert_grid: null query", q=None)
    for kw, why in SOLVER_REFUSALS:
        refused("lambert_grid: " + why, **kw)
    for mu in (0.0, -1.0, float("nan"), float("inf")):
        refused("lambert_grid: mu_km3_s2 must be finite and > 0", mu_km3_s2=mu)
    refused("n_dep = -1, n_arr = 3", n_dep=-1)
    refused("n_dep = 2, n_arr = -4", n_arr=-4)
    refused("n_dep = 2147483648", n_dep=2**31)
    refused("has_tof = 2, 0 or 1", has_tof=2)
    refused("dep_step_ns must be > 0", dep_step_ns=0)
    refused("arr_step_ns must be > 0", arr_step_ns=-1)
    refused("tof_step_ns must be > 0", has_tof=1, tof_step_ns=0)
    refused("values and status arrays required", v=None)
    refused("values and status arrays required", s=None)
    refused("dep.n_chain = 5, 0 .. 4 segments", dep=dict(n_chain=5))
    refused("arr.n_chain = -1", arr=dict(n_chain=-1))
    refused("centre.chain_segment[0] = -2 is not a segment of the context", centre=dict(chain_segment=(0, -2)))
    refused("arr.chain_sign[1] = 0, +1 or -1", arr=dict(chain_sign=(1, 0)))
    refused("dep.chain_sign[0] = 2", dep=dict(chain_sign=(0, 2)))
    refused("the departure body's chain is the centre's", dep=dict(n_chain=1, chain_segment=(0, 1), chain_sign=(0, -1)))
    refused("the arrival body's chain is the centre's", arr=dict(n_chain=1, chain_segment=(0, 1), chain_sign=(0, -1)))
    refused("the departure body's chain is the centre's", dep=dict(n_chain=0), centre=dict(n_chain=0))
    refused("lambert_grid: way = 5", way=5, n_dep=-1, dep=dict(n_chain=9))     # the solver first, then the sizes, then the chains
    refused("n_dep = -1", n_dep=-1, dep=dict(n_chain=9), v=None)
    refused("arrays required", v=None, dep=dict(n_chain=9))
    assert (values == 0).all() and (status == 0).all()


def test_the_context_is_asked_behind_the_query_alone():
    src = open(os.path.join(ROOT, "nyx_amd", "csrc", "abi.cpp")).read()
    body = src[src.index("static Refusal check_lambert("):]
    body = body[:body.index("\n}\n")]
    assert body.index("check_lambert_grid(ctx, q, values, status)") < body.index("check_lambert_context(*q, ctx->host_cfg.n_seg, ctx->swap_n_chain != 0)")
    for entry in ("nyx_hip_lambert_grid_device", "nyx_hip_lambert_grid"):
        fn = src[src.index(f'extern "C" int32_t {entry}('):]
        fn = fn[fn.index("{") + 1:fn.index("\n}\n")]
        assert fn.lstrip().startswith("if (Refusal r = check_lambert(ctx, q, values, status)) return refused(r);"), entry
    for entry in ("nyx_hip_lambert_batch_device", "nyx_hip_lambert_batch"):
        fn = src[src.index(f'extern "C" int32_t {entry}('):]
        fn = fn[fn.index("{") + 1:fn.index("\n}\n")]
        assert fn.lstrip().startswith("if (Refusal r = check_lambert_batch(ctx, rv1, rv2, tof_s, n, mu_km3_s2, q, values, status)) return refused(r);"), entry
    args = open(os.path.join(ROOT, "nyx_amd", "csrc", "lambert_args.h")).read()
    assert "NYX_HIP_RC_UNSUPPORTED" in args[args.index("inline Refusal check_lambert_context("):] and "hip_runtime" not in args


def test_c_and_cxx_programs_compile_and_link(tmp_path):
    """include/nyx_hip_lambert.h from C, include/nyx_hip_lambert.hpp from C++: syntax alone, then against the built library (host only:
    the layout check runs, nothing is launched)."""
    _abi.load_library()
    inc = "-I" + os.path.join(ROOT, "include")
    link = ["-L" + os.path.join(ROOT, "nyx_amd"), "-lnyx_hip", "-Wl,-rpath," + os.path.join(ROOT, "nyx_amd")]
    c_src = tmp_path / "lmb_check.c"
    c_src.write_text('#include "nyx_hip_lambert.h"\n'
                     "int main(void) { nyx_hip_lambert_grid_query_t q; q.n_dep = 0; (void)q;\n"
                     "    return nyx_hip_lambert_sizeof(0) == (int32_t)sizeof(nyx_hip_lambert_query_t) && nyx_hip_lambert_sizeof(2) == NYX_HIP_LMB_COUNT &&\n"
                     "           nyx_hip_lambert_sizeof(4) == (int32_t)sizeof(nyx_hip_lambert_grid_query_t) && nyx_hip_lambert_sizeof(1) == NYX_HIP_LAMBERT_VERSION ? 0 : 1; }\n")
    exe = str(tmp_path / "lmb_check_c")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", inc, str(c_src), *link, "-o", exe], check=True)
    assert subprocess.run([exe]).returncode == 0
    src = tmp_path / "lmb_check.cpp"
    src.write_text('#include "nyx_hip_lambert.hpp"\n'
                   "nyx::LambertGrid porkchop(nyx::GpuPropagator &p, const nyx_hip_lambert_grid_query_t &q) {\n"
                   "    nyx::LambertSolver s; s.way = NYX_HIP_LMB_SHORT;\n"
                   "    return nyx::lambert_grid(p, q, {NYX_HIP_LMB_C3, NYX_HIP_LMB_VINF_ARR, NYX_HIP_LMB_DLA_DEG, NYX_HIP_LMB_TOF_S}, s);\n"
                   "}\n"
                   "nyx::LambertGrid batch(nyx::GpuPropagator &p, const std::vector<double> &a, const std::vector<double> &b, const std::vector<double> &t) {\n"
                   "    return nyx::lambert_batch(p, a, b, t, 398600.4, {NYX_HIP_LMB_V1X, NYX_HIP_LMB_V1Y, NYX_HIP_LMB_V1Z});\n"
                   "}\n"
                   "int main() { return nyx_hip_lambert_sizeof(5) == (int32_t)sizeof(nyx_hip_lambert_chain_t) && NYX_HIP_LMB_COUNT == 16 &&\n"
                   "             nyx_hip_lambert_sizeof(3) == NYX_HIP_MAX_LAMBERT_PARAMS ? 0 : 1; }\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", inc, str(src)], check=True)
    exe = str(tmp_path / "lmb_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", inc, str(src), *link, "-o", exe], check=True)
    assert subprocess.run([exe]).returncode == 0
