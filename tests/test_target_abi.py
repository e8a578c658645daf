"""CPU checks of the targeter's boundary (include/nyx_hip_target.h), the twin of tests/test_lambert_abi.py: every declared function is
exported by the built library, the struct layouts and the codes match the ctypes mirrors and the enums of nyx_amd/targeter.py, every
refusal that can be told from the arguments alone is given before a device is touched - by both flavours, the outputs left untouched,
in the order the header lists them -, and a C and a C++ program that include only the new headers compile and link.  No compute calls
(no GPU here).  What a query asks OF THE CONTEXT - a segment index beyond the context's, a context with STMs or the integration-frame
swap - needs a context, which needs a device; here the source of abi.cpp is held to the chaining."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from nyx_amd import _abi, targeter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nyx_hip_target.h")


def _fields(header, struct):
    body = re.search(r"typedef struct %s \{(.*?)\} %s_t;" % (struct, struct), header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        if decl.strip():
            names = re.sub(r"^\s*(?:const\s+)?\w+\s+", "", decl.strip())
            out += [re.sub(r"\[.*", "", n.strip().lstrip("*")) for n in names.split(",")]
    return out


def test_every_declared_target_function_is_exported():
    lib = _abi.load_library()
    declared = set(re.findall(r"^(?:int32_t|void|double|const char \*)\s*(nyx_hip_[a-z_0-9]+)\(", open(HEADER).read(), flags=re.M))
    assert declared == {"nyx_hip_target_batch", "nyx_hip_target_batch_device", "nyx_hip_target_sizeof"} == set(_abi.TARGET_EXPORTS)
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in nyx_hip_target.h but not exported"
        assert _abi.target_entry(lib, name) is getattr(lib, name)
    others = (_abi.EXPORTS, _abi.REPORT_EXPORTS, _abi.RIC_EXPORTS, _abi.GROUNDTRACK_EXPORTS, _abi.AER_EXPORTS, _abi.ECLIPSE_EXPORTS, _abi.FRAME_EXPORTS,
              _abi.LINK_EXPORTS, _abi.LAMBERT_EXPORTS, _abi.STATS_EXPORTS)
    assert not any(declared & set(o) for o in others)
    # nyx_hip.h does not know them: NYX_HIP_ABI_VERSION and its declaration list are unchanged
    main = open(os.path.join(ROOT, "include", "nyx_hip.h")).read()
    assert "nyx_hip_target" not in main and "NYX_HIP_TGT" not in main and "NYX_HIP_VARY" not in main and _abi.ABI_VERSION == 4

    class Old:   # a library built before the targeter: no such symbol
        pass

    with pytest.raises(RuntimeError, match="has no nyx_hip_target_batch.*rebuild"):
        _abi.target_entry(Old())


def test_layouts_and_codes_match_the_header():
    lib = _abi.load_library()
    header = open(HEADER).read()
    assert lib.nyx_hip_target_sizeof(0) == C.sizeof(_abi.TargetQuery) == 16 + 24 + 5 * 48 + 24 + 4 * 48 + 40 + 8 + 16 == 560
    assert lib.nyx_hip_target_sizeof(4) == C.sizeof(_abi.TargetResult) == 4 * 8 + 2 * C.sizeof(_abi.States) + 8 == 312
    assert lib.nyx_hip_target_sizeof(1) == _abi.TARGET_VERSION == int(re.search(r"#define NYX_HIP_TARGET_VERSION (\d+)", header).group(1))
    assert lib.nyx_hip_target_sizeof(3) == _abi.MAX_TARGET_VARS == targeter.MAX_VARS == int(re.search(r"#define NYX_HIP_MAX_TARGET_VARS (\d+)", header).group(1)) == 6
    assert lib.nyx_hip_target_sizeof(5) == _abi.MAX_TARGET_OBJS == targeter.MAX_OBJS == int(re.search(r"#define NYX_HIP_MAX_TARGET_OBJS (\d+)", header).group(1)) == 6
    assert int(re.search(r"#define NYX_HIP_TARGET_MAX_ITERATIONS (\d+)", header).group(1)) == targeter.MAX_ITERATIONS == 1000
    assert lib.nyx_hip_target_sizeof(6) == -1 and lib.nyx_hip_target_sizeof(-1) == -1
    for struct, mirror in (("nyx_hip_target_query", _abi.TargetQuery), ("nyx_hip_target_result", _abi.TargetResult)):
        assert _fields(header, struct) == [f for f, _ in mirror._fields_], struct
    names = [f for f, _ in _abi.TargetQuery._fields_]
    assert [getattr(_abi.TargetQuery, f).offset for f in names] == [0, 4, 8, 12, 16, 40, 88, 136, 184, 232, 280, 304, 352, 400, 448, 496, 500, 516, 532, 536, 544, 552]
    # the enums are pinned: never renumbered
    codes = dict((k, int(v)) for k, v in re.findall(r"NYX_HIP_TGT_([A-Z_]+) = (\d+)", header))
    assert {k: v for k, v in codes.items() if k != "STATUS_COUNT"} == _abi.TARGET_STATUS == {s.name: int(s) for s in targeter.TargetStatus}
    assert codes["STATUS_COUNT"] == lib.nyx_hip_target_sizeof(2) == _abi.TARGET_STATUS_COUNT == len(targeter.TargetStatus) == 7
    vary = dict((k, int(v)) for k, v in re.findall(r"NYX_HIP_VARY_([A-Z_]+) = (\d+)", header))
    assert [vary[k] for k in ("POSITION_X", "POSITION_Y", "POSITION_Z", "VELOCITY_X", "VELOCITY_Y", "VELOCITY_Z", "COUNT")] == list(range(7))
    assert [int(v) for v in targeter.Vary] == list(range(6)) and (_abi.FRAME_INERTIAL, _abi.FRAME_VNC) == (0, 2)
    d = targeter.Variable(targeter.Vary.VelocityX)
    assert (d.perturbation, d.init_guess, d.max_step, d.max_value, d.min_value) == (1e-4, 0.0, 0.2, 5.0, -5.0)


def good_query(**kw):
    q = _abi.TargetQuery()
    q.n_vars, q.n_objs, q.iterations, q.correction_frame, q.mu_km3_s2 = 3, 2, 100, 0, 398600.4
    for j in range(3):
        q.var_component[j], q.var_perturbation[j], q.var_max_step[j], q.var_max_value[j], q.var_min_value[j] = 3 + j, 1e-4, 0.2, 5.0, -5.0
    for o, (p, want, tol) in enumerate(((11, 0.4, 1e-5), (10, 8100.0, 0.1))):
        q.obj_param[o], q.obj_desired[o], q.obj_tolerance[o], q.obj_mult[o] = p, want, tol, 1.0
    q.n_chain = 2
    q.chain_segment[0], q.chain_sign[0], q.chain_segment[1], q.chain_sign[1] = 3, 1, 2, -1
    for k, v in kw.items():
        if isinstance(v, tuple):
            getattr(q, k)[v[0]] = v[1]
        else:
            setattr(q, k, v)
    return q


NAN, INF = float("nan"), float("inf")
REFUSALS = [(dict(n_vars=0), "n_vars = 0, 1 .. 6 variables"), (dict(n_vars=7), "n_vars = 7"), (dict(n_objs=0), "n_objs = 0, 1 .. 6 objectives"),
            (dict(n_objs=7), "n_objs = 7"), (dict(iterations=-1), "iterations = -1, 0 .. 1000"), (dict(iterations=1001), "iterations = 1001"),
            (dict(correction_frame=1), "correction_frame = 1, inertial (0) or VNC (2)"), (dict(correction_frame=3), "correction_frame = 3"),
            (dict(var_component=(1, 6)), "var_component[1] = 6 is not a nyx_hip_target_vary"), (dict(var_component=(0, -1)), "var_component[0] = -1"),
            (dict(var_perturbation=(2, 0.0)), "var_perturbation[2] must be finite and not zero"), (dict(var_perturbation=(0, NAN)), "var_perturbation[0]"),
            (dict(var_perturbation=(0, INF)), "var_perturbation[0]"), (dict(var_init_guess=(1, NAN)), "var_init_guess[1] must be finite"),
            (dict(var_max_step=(0, -0.1)), "var_max_step[0] must be >= 0"), (dict(var_max_step=(0, NAN)), "var_max_step[0]"),
            (dict(var_max_value=(1, -1.0)), "var_max_value[1] must be >= 0"), (dict(var_min_value=(2, 6.0)), "var_min_value[2] must be <= var_max_value[2]"),
            (dict(correction_frame=2, var_component=(0, 1)), "var_component[0] is a position"),
            (dict(obj_param=(0, 25)), "obj_param[0] = 25 is not a nyx_hip_frame_param"), (dict(obj_param=(1, -1)), "obj_param[1] = -1"),
            (dict(obj_tolerance=(0, -1e-9)), "obj_tolerance[0] must be finite and >= 0"), (dict(obj_tolerance=(1, INF)), "obj_tolerance[1]"),
            (dict(obj_tolerance=(1, NAN)), "obj_tolerance[1]"), (dict(obj_desired=(0, NAN)), "obj_desired[0]"),
            (dict(n_chain=5), "n_chain = 5, 0 .. 4 segments"), (dict(n_chain=-1), "n_chain = -1"),
            (dict(chain_segment=(1, -2)), "chain_segment[1] = -2 is not a segment of the context"), (dict(chain_sign=(0, 0)), "chain_sign[0] = 0, +1 or -1"),
            (dict(mu_km3_s2=0.0), "mu_km3_s2 must be finite and > 0"), (dict(mu_km3_s2=NAN), "mu_km3_s2"), (dict(mu_km3_s2=INF), "mu_km3_s2"),
            # which check wins: the first of the header's list
            (dict(n_vars=0, n_objs=0, iterations=-1), "n_vars = 0"), (dict(n_objs=9, iterations=-1, correction_frame=7), "n_objs = 9"),
            (dict(iterations=2000, correction_frame=7), "iterations = 2000"), (dict(correction_frame=7, var_component=(0, 9)), "correction_frame = 7"),
            (dict(var_perturbation=(0, 0.0), var_component=(1, 9)), "var_perturbation[0]"), (dict(var_max_step=(2, -1.0), obj_param=(0, 99)), "var_max_step[2]"),
            (dict(obj_param=(0, 99), n_chain=9, mu_km3_s2=0.0), "obj_param[0] = 99"), (dict(n_chain=9, mu_km3_s2=0.0), "n_chain = 9"),
            # a seventh entry is not read
            ]


def test_bad_problems_are_refused_before_any_device_is_touched():
    lib = _abi.load_library()
    n = 2
    batch = _abi.StateBatch(n)
    status, its = np.full(n, -7, dtype=np.int32), np.full(n, -7, dtype=np.int32)
    corr, errs = np.full(6 * n, 123.0), np.full(6 * n, 123.0)
    corrected, achieved = _abi.StateBatch(n), _abi.StateBatch(n)
    for b in (corrected, achieved):
        b.set_rv(np.full((n, 6), 123.0))
    fake_ctx = C.c_void_p(1)   # never dereferenced: every case below fails on the arguments alone

    def result(**kw):
        r = _abi.TargetResult()
        r.status, r.iterations = status.ctypes.data_as(_abi.c_int32_p), its.ctypes.data_as(_abi.c_int32_p)
        r.correction, r.achieved_errors = corr.ctypes.data_as(_abi.c_double_p), errs.ctypes.data_as(_abi.c_double_p)
        r.corrected, r.achieved = corrected.as_c(), achieved.as_c()
        r.iterations_run = -7
        for k, v in kw.items():
            if "." in k:
                setattr(getattr(r, k.split(".")[0]), k.split(".")[1], v)
            else:
                setattr(r, k, v)
        return r

    def refused(why, ctx=fake_ctx, q="default", cin="default", res="default", rc_want=_abi.RC_BAD_ARG, res_kw=None, **kw):
        q = good_query(**kw) if q == "default" else q
        cin = batch.as_c() if cin == "default" else cin
        res = result(**(res_kw or {})) if res == "default" else res
        refs = [C.byref(x) if x is not None else None for x in (cin, q, res)]
        for rc in (lib.nyx_hip_target_batch(ctx, *refs), lib.nyx_hip_target_batch_device(ctx, *refs, None)):
            assert rc == rc_want and why in _abi.last_error(), (why, rc, _abi.last_error())
        assert res is None or res.iterations_run == -7

    refused("null ctx", ctx=None)
    refused("target_batch: null query", q=None)
    refused("target_batch: null result", res=None)
    for kw, why in REFUSALS:
        refused("target_batch: " + why, **kw)
    bad_in = batch.as_c()
    bad_in.vz_km_s = _abi.c_double_p()
    refused("in: epoch and the six Cartesian arrays are mandatory", cin=bad_in)
    refused("in: epoch and the six Cartesian arrays are mandatory", cin=None)
    neg = batch.as_c()
    neg.n = -1
    refused("in: epoch", cin=neg)
    refused("mu_km3_s2", cin=bad_in, mu_km3_s2=0.0)        # the query before the batch
    for f in ("status", "iterations", "correction", "achieved_errors"):
        refused("status, iterations, correction and achieved_errors arrays required", res_kw={f: None})
    refused("corrected and achieved: epoch and the six Cartesian arrays are mandatory", res_kw={"corrected.x_km": _abi.c_double_p()})
    refused("corrected and achieved: epoch and the six Cartesian arrays are mandatory", res_kw={"achieved.epoch_ns": _abi.c_int64_p()})
    refused("in: epoch", cin=bad_in, res_kw={"status": None})   # the batch before the outputs
    with_stm = _abi.StateBatch(n, with_stm=True).as_c()
    refused("in->stm is given: the hyperdual targeter", cin=with_stm, rc_want=_abi.RC_UNSUPPORTED)
    refused("arrays required", cin=with_stm, res_kw={"status": None})   # BAD_ARG wins over UNSUPPORTED
    # the outputs were left untouched
    assert (status == -7).all() and (its == -7).all() and (corr == 123.0).all() and (errs == 123.0).all()
    assert (corrected.rv() == 123.0).all() and (achieved.rv() == 123.0).all()


def test_the_context_is_asked_behind_the_query_alone():
    src = open(os.path.join(ROOT, "nyx_amd", "csrc", "abi.cpp")).read()
    body = src[src.index("static Refusal check_tgt("):]
    body = body[:body.index("\n}\n")]
    assert body.index("check_target(ctx, in, q, res)") < body.index("check_target_context(*q, ctx->host_cfg.n_seg")
    for entry in ("nyx_hip_target_batch_device", "nyx_hip_target_batch"):
        fn = src[src.index(f'extern "C" int32_t {entry}('):]
        fn = fn[fn.index("{") + 1:fn.index("\n}\n")]
        assert fn.lstrip().startswith("if (Refusal r = check_tgt(ctx, in, q, res)) return refused(r);"), entry
        assert "CTX_LOCK(ctx);" in fn
    args = open(os.path.join(ROOT, "nyx_amd", "csrc", "target_args.h")).read()
    assert args[args.index("inline Refusal check_target_context("):].count("NYX_HIP_RC_UNSUPPORTED") == 1 and "hip_runtime" not in args
    # the loop reads four bytes per round and nothing else
    loop = src[src.index("for (int it = 0; it <= q->iterations; ++it)"):]
    loop = loop[:loop.index("\n    }\n")]
    assert loop.count("hipMemcpyAsync") == 1 and "sizeof live" in loop and "hipStreamSynchronize(stream)" in loop


def test_c_and_cxx_programs_compile_and_link(tmp_path):
    """include/nyx_hip_target.h from C, include/nyx_hip_target.hpp from C++: syntax alone, then against the built library (host only:
    the layout check runs, nothing is launched)."""
    _abi.load_library()
    inc = "-I" + os.path.join(ROOT, "include")
    link = ["-L" + os.path.join(ROOT, "nyx_amd"), "-lnyx_hip", "-Wl,-rpath," + os.path.join(ROOT, "nyx_amd")]
    c_src = tmp_path / "tgt_check.c"
    c_src.write_text('#include "nyx_hip_target.h"\n'
                     "int main(void) { nyx_hip_target_query_t q; q.n_vars = 0; (void)q;\n"
                     "    return nyx_hip_target_sizeof(0) == (int32_t)sizeof(nyx_hip_target_query_t) && nyx_hip_target_sizeof(2) == NYX_HIP_TGT_STATUS_COUNT &&\n"
                     "           nyx_hip_target_sizeof(4) == (int32_t)sizeof(nyx_hip_target_result_t) && nyx_hip_target_sizeof(1) == NYX_HIP_TARGET_VERSION ? 0 : 1; }\n")
    exe = str(tmp_path / "tgt_check_c")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", inc, str(c_src), *link, "-o", exe], check=True)
    assert subprocess.run([exe]).returncode == 0
    src = tmp_path / "tgt_check.cpp"
    src.write_text('#include "nyx_hip_target.hpp"\n'
                   "nyx::TargeterSolutions correct(nyx::GpuPropagator &p, nyx::StateBatch &b, const nyx_hip_target_query_t &q) {\n"
                   "    nyx::TargetVariable vx, vy; vy.component = NYX_HIP_VARY_VELOCITY_Y; vy.max_step = 0.5;\n"
                   "    nyx::TargetObjective sma; sma.param = NYX_HIP_SP_SEMI_MAJOR_AXIS; sma.desired = 8100.0; sma.tolerance = 0.1;\n"
                   "    return nyx::target_batch(p, b, q, {vx, vy}, {sma});\n"
                   "}\n"
                   "int main() { return nyx_hip_target_sizeof(3) == NYX_HIP_MAX_TARGET_VARS && NYX_HIP_TGT_EPHEM_RANGE == 6 &&\n"
                   "             nyx_hip_target_sizeof(5) == NYX_HIP_MAX_TARGET_OBJS ? 0 : 1; }\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", inc, str(src)], check=True)
    exe = str(tmp_path / "tgt_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", inc, str(src), *link, "-o", exe], check=True)
    assert subprocess.run([exe]).returncode == 0
