"""CPU checks of the eclipse boundary (include/nyx_hip_eclipse.h), the twin of tests/test_aer_abi.py: every declared function is
exported by the built library, the struct layouts and the parameter codes match the ctypes mirror, every member of
`EclipseParameter` has a code, every refusal that can be told from the query alone is given before a device is touched - by both
flavours, the outputs left untouched ("nothing is launched then") -, the Python layer refuses what the device path refuses, and the
C++ wrapper compiles.  No compute calls (no GPU here).  What a query asks OF THE CONTEXT - a segment index beyond the context's
segments, the integration-frame swap refused with NYX_HIP_RC_UNSUPPORTED - needs a context, which needs a device: the rule itself
(`check_ecl_context` of csrc/series_host.h, chained behind `check_ecl_series` exactly as abi.cpp chains them) is run by the
stand-alone program of tests/test_eclipse_host_cxx.py, and through the library on the GPU by tests/test_gpu_eclipse.py; here the
source of abi.cpp is held to that chaining."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import nyx_amd as nx
from nyx_amd import _abi
from nyx_amd.eclipse import EclipseParameter as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nyx_hip_eclipse.h")


def _declared():
    return set(re.findall(r"^(?:int32_t|void|double|const char \*)\s*(nyx_hip_[a-z_0-9]+)\(", open(HEADER).read(), flags=re.M))


def _fields(header, struct):
    body = re.search(r"typedef struct %s \{(.*?)\} %s_t;" % (struct, struct), header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [re.sub(r"\[.*", "", n.strip()) for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]


def test_every_declared_eclipse_function_is_exported():
    lib = _abi.load_library()
    declared = _declared()
    assert declared == {"nyx_hip_traj_eclipse", "nyx_hip_traj_eclipse_device", "nyx_hip_ecl_sizeof"}
    assert declared == set(_abi.ECLIPSE_EXPORTS)
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in nyx_hip_eclipse.h but not exported"
        assert _abi.eclipse_entry(lib, name) is getattr(lib, name)
    # the entries stay out of the lists of the other headers (the Rust block is generated against EXPORTS)
    assert not declared & (set(_abi.EXPORTS) | set(_abi.REPORT_EXPORTS) | set(_abi.RIC_EXPORTS) | set(_abi.GROUNDTRACK_EXPORTS) | set(_abi.AER_EXPORTS))
    # and nyx_hip.h does not know them: NYX_HIP_ABI_VERSION and its declaration list are unchanged
    assert "nyx_hip_ecl" not in open(os.path.join(ROOT, "include", "nyx_hip.h")).read() and "nyx_hip_traj_eclipse" not in open(os.path.join(ROOT, "include", "nyx_hip.h")).read()


def test_an_older_library_gives_a_clear_error():
    class Old:   # a library built before the eclipses: no such symbol
        pass

    with pytest.raises(RuntimeError, match="has no nyx_hip_traj_eclipse.*rebuild"):
        _abi.eclipse_entry(Old())


def test_query_layout_and_constants_match_the_header():
    lib = _abi.load_library()
    header = open(HEADER).read()
    assert lib.nyx_hip_ecl_sizeof(5) == C.sizeof(_abi.EclBody) == 4 + 16 + 16 + 4 + 8 == 48
    assert lib.nyx_hip_ecl_sizeof(0) == C.sizeof(_abi.EclQuery) == 4 + 32 + 32 + 4 + 3 * 8 + 48 + 8 + 8 * 48 == 536
    assert lib.nyx_hip_ecl_sizeof(1) == _abi.ECL_VERSION == int(re.search(r"#define NYX_HIP_ECL_VERSION (\d+)", header).group(1))
    assert lib.nyx_hip_ecl_sizeof(3) == _abi.MAX_ECL_PARAMS == int(re.search(r"#define NYX_HIP_MAX_ECL_PARAMS (\d+)", header).group(1)) == 8
    assert lib.nyx_hip_ecl_sizeof(4) == _abi.MAX_ECL_BODIES == int(re.search(r"#define NYX_HIP_MAX_ECL_BODIES (\d+)", header).group(1)) == 8
    assert lib.nyx_hip_ecl_sizeof(6) == -1 and lib.nyx_hip_ecl_sizeof(-1) == -1
    # field order of the mirrors = field order of the header
    assert _fields(header, "nyx_hip_ecl_query") == [f for f, _ in _abi.EclQuery._fields_]
    assert _fields(header, "nyx_hip_ecl_body") == [f for f, _ in _abi.EclBody._fields_] == ["n_chain", "chain_segment", "chain_sign", "_pad", "mean_radius_km"]
    assert [getattr(_abi.EclQuery, f).offset for f in ("param", "param_body", "has_window", "step_ns", "light", "n_bodies", "bodies")] == [4, 36, 68, 72, 96, 144, 152]
    assert _abi.MAX_CHAIN == int(re.search(r"#define NYX_HIP_MAX_CHAIN (\d+)", open(os.path.join(ROOT, "include", "nyx_hip.h")).read()).group(1))


def test_parameter_codes_match_the_header_and_cover_the_enum():
    lib = _abi.load_library()
    header = open(HEADER).read()
    enum = dict((k, int(v)) for k, v in re.findall(r"NYX_HIP_ECL_([A-Z_]+) = (\d+)", header))
    count = enum.pop("COUNT")
    assert count == len(enum) == 11 == lib.nyx_hip_ecl_sizeof(2)
    assert sorted(enum.values()) == list(range(11))
    assert {re.sub(r"(?<!^)(?=[A-Z])", "_", name).upper(): code for name, code in _abi.ECL_PARAM.items()} == enum
    assert {p.name: int(p) for p in E} == _abi.ECL_PARAM
    assert _abi.ECL_FIRST_PER_BODY == int(E.BodyOccultation) == min(int(p) for p in nx.eclipse.PER_BODY)
    model = nx.ShadowModel(nx.Frame(nx.SUN, 1.0, 696000.0), [nx.Frame(nx.EARTH, 1.0, 6378.0), nx.Frame(nx.MOON, 1.0, 1737.4)])
    for p in E:
        if p in nx.eclipse.PER_BODY:
            assert nx.ecl_param_code((p, model.shadow_bodies[1]), model) == (_abi.ECL_PARAM[p.name], 1) == nx.ecl_param_code((p, 1), model)
            with pytest.raises(ValueError, match="per-body"):
                nx.ecl_param_code(p, model)
        else:
            assert nx.ecl_param_code(p, model) == (_abi.ECL_PARAM[p.name], 0)
            with pytest.raises(ValueError, match="takes no body"):
                nx.ecl_param_code((p, 0), model)
    with pytest.raises(ValueError, match="not a shadow body"):
        nx.ecl_param_code((E.BodyOccultation, nx.Frame(nx.JUPITER_BARYCENTER, 1.0, 7e4)), model)
    with pytest.raises(TypeError):     # a station-view parameter is not an eclipse parameter
        nx.ecl_param_code(nx.AerParameter.Range, model)


def test_bad_queries_are_refused_before_any_device_is_touched():
    """Argument validation comes first: the same answer with and without a GPU, and never a clipped request."""
    lib = _abi.load_library()
    t = _abi.TrajBatch(2, 4)
    ct = t.as_c()
    values, length = np.zeros(8 * 4 * 2), np.zeros(2, dtype=np.int32)
    vp, lp = values.ctypes.data_as(_abi.c_double_p), length.ctypes.data_as(_abi.c_int32_p)
    fake_ctx = C.c_void_p(1)   # never dereferenced: every case below fails on the query alone
    nan, inf = float("nan"), float("inf")

    def query(n_params=1, param=_abi.ECL_PARAM["Occultation"], param_body=0, step=10**9, n_bodies=2, light=None, body=None, at=1):
        q = _abi.EclQuery()
        q.n_params, q.step_ns, q.n_bodies = n_params, step, n_bodies
        for k in range(8):
            q.param[k], q.param_body[k] = param, param_body
        q.light.n_chain, q.light.mean_radius_km = 3, 696000.0
        for k, (seg, sign) in enumerate([(2, 1), (1, -1), (0, -1)]):
            q.light.chain_segment[k], q.light.chain_sign[k] = seg, sign
        for b in range(8):
            q.bodies[b].n_chain, q.bodies[b].mean_radius_km = 2, 1737.4
            for k, (seg, sign) in enumerate([(3, 1), (0, -1)]):
                q.bodies[b].chain_segment[k], q.bodies[b].chain_sign[k] = seg, sign
        q.bodies[0].n_chain, q.bodies[0].mean_radius_km = 0, 6378.14
        for target, changes in ((q.light, light), (q.bodies[at], body)):
            for f, v in (changes or {}).items():
                if isinstance(v, tuple):
                    getattr(target, f)[v[0]] = v[1]
                else:
                    setattr(target, f, v)
        return q

    def refused(ctx, q, capacity, v, l, why, n=2):
        rc = lib.nyx_hip_traj_eclipse(ctx, C.byref(ct), n, C.byref(q) if q is not None else None, capacity, v, l)
        assert rc == _abi.RC_BAD_ARG and why in _abi.last_error(), (rc, _abi.last_error())
        rc = lib.nyx_hip_traj_eclipse_device(ctx, C.byref(ct), n, C.byref(q) if q is not None else None, capacity, v, l, None)
        assert rc == _abi.RC_BAD_ARG and why in _abi.last_error(), (rc, _abi.last_error())

    refused(None, query(), 4, vp, lp, "null ctx")
    refused(fake_ctx, None, 4, vp, lp, "null query")
    refused(fake_ctx, query(n_params=0), 4, vp, lp, "n_params = 0")
    refused(fake_ctx, query(n_params=9), 4, vp, lp, "n_params = 9")
    refused(fake_ctx, query(param=11), 4, vp, lp, "param[0] = 11 is not a nyx_hip_ecl_param")
    refused(fake_ctx, query(param=-1), 4, vp, lp, "param[0] = -1")
    refused(fake_ctx, query(step=0), 4, vp, lp, "step_ns must be > 0")
    refused(fake_ctx, query(step=-5), 4, vp, lp, "step_ns must be > 0")
    refused(fake_ctx, query(), 0, vp, lp, "capacity")
    refused(fake_ctx, query(), 4, vp, lp, "negative n", n=-1)
    refused(fake_ctx, query(), 4, None, lp, "values and len arrays required")
    refused(fake_ctx, query(), 4, vp, None, "values and len arrays required")
    refused(fake_ctx, query(n_bodies=0), 4, vp, lp, "n_bodies = 0")
    refused(fake_ctx, query(n_bodies=-1), 4, vp, lp, "n_bodies = -1")
    refused(fake_ctx, query(n_bodies=9), 4, vp, lp, "n_bodies = 9")
    refused(fake_ctx, query(light={"n_chain": 0}), 4, vp, lp, "light.n_chain = 0, 1 .. 4")
    refused(fake_ctx, query(light={"n_chain": 5}), 4, vp, lp, "light.n_chain = 5")
    refused(fake_ctx, query(light={"chain_segment": (1, -1)}), 4, vp, lp, "light.chain_segment[1] = -1")
    refused(fake_ctx, query(light={"chain_sign": (2, 0)}), 4, vp, lp, "light.chain_sign[2] = 0")
    refused(fake_ctx, query(light={"mean_radius_km": 0.0}), 4, vp, lp, "light.mean_radius_km")
    refused(fake_ctx, query(light={"mean_radius_km": nan}), 4, vp, lp, "light.mean_radius_km")
    refused(fake_ctx, query(body={"n_chain": -1}), 4, vp, lp, "bodies[1].n_chain = -1, 0 .. 4")
    refused(fake_ctx, query(body={"n_chain": 5}, at=0), 4, vp, lp, "bodies[0].n_chain = 5")
    refused(fake_ctx, query(body={"chain_segment": (0, -3)}), 4, vp, lp, "bodies[1].chain_segment[0] = -3")
    refused(fake_ctx, query(body={"chain_sign": (1, 2)}), 4, vp, lp, "bodies[1].chain_sign[1] = 2")
    refused(fake_ctx, query(body={"mean_radius_km": inf}), 4, vp, lp, "bodies[1].mean_radius_km")
    refused(fake_ctx, query(body={"mean_radius_km": -1.0}, n_bodies=8, at=7), 4, vp, lp, "bodies[7].mean_radius_km")
    refused(fake_ctx, query(param=_abi.ECL_PARAM["BodyUmbraMargin"], param_body=2), 4, vp, lp, "param_body[0] = 2")
    refused(fake_ctx, query(param=_abi.ECL_PARAM["BodyOccultation"], param_body=-1), 4, vp, lp, "param_body[0] = -1")
    assert (values == 0).all() and (length == 0).all()


def test_the_context_is_asked_behind_the_query_alone():
    """abi.cpp chains check_ecl_series (never reads the context) and check_ecl_context (its segments, no frame swap), in that order,
    in front of everything that touches a device - in both flavours."""
    src = open(os.path.join(ROOT, "nyx_amd", "csrc", "abi.cpp")).read()
    body = src[src.index("static Refusal check_ecl("):]
    body = body[:body.index("\n}\n")]
    assert body.index("check_ecl_series(ctx, traj, n, q, capacity, values, len)") < body.index("check_ecl_context(*q, ctx->host_cfg.n_seg, ctx->swap_n_chain != 0)")
    for entry in ("nyx_hip_traj_eclipse_device", "nyx_hip_traj_eclipse"):
        fn = src[src.index(f'extern "C" int32_t {entry}('):]
        fn = fn[fn.index("{") + 1:fn.index("\n}\n")]
        assert fn.lstrip().startswith("if (Refusal r = check_ecl(ctx, traj, n, q, capacity, values, len)) return refused(r);"), entry
    host = open(os.path.join(ROOT, "nyx_amd", "csrc", "series_host.h")).read()
    assert "NYX_HIP_RC_UNSUPPORTED" in host[host.index("inline Refusal check_ecl_context("):] and "integration-frame swap" in host


def test_cxx_wrapper_compiles_and_links(tmp_path):
    """include/nyx_hip_eclipse.hpp: syntax alone, then against the built library (host only: the layout check runs, nothing is
    launched)."""
    _abi.load_library()
    src = tmp_path / "ecl_check.cpp"
    src.write_text('#include "nyx_hip_eclipse.hpp"\n'
                   "nyx::EclipseSeries shadow(nyx::GpuPropagator &p, nyx::TrajBatch &t, const nyx::ShadowModel &m) {\n"
                   "    return nyx::traj_eclipse(p, t, m, {{NYX_HIP_ECL_OCCULTATION, 0}, {NYX_HIP_ECL_STATE, 0}, {NYX_HIP_ECL_BODY_PENUMBRA_MARGIN, 1}},\n"
                   "                             60000000000LL, 1441);\n"
                   "}\n"
                   "int main() { return nyx_hip_ecl_sizeof(0) == (int32_t)sizeof(nyx_hip_ecl_query_t) && NYX_HIP_ECL_COUNT == 11 &&\n"
                   "             nyx_hip_ecl_sizeof(5) == (int32_t)sizeof(nyx_hip_ecl_body_t) && nyx_hip_ecl_sizeof(4) == NYX_HIP_MAX_ECL_BODIES ? 0 : 1; }\n")
    inc = "-I" + os.path.join(ROOT, "include")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", inc, str(src)], check=True)
    exe = str(tmp_path / "ecl_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", inc, str(src), "-L" + os.path.join(ROOT, "nyx_amd"),
                    "-lnyx_hip", "-Wl,-rpath," + os.path.join(ROOT, "nyx_amd"), "-o", exe], check=True)
    assert subprocess.run([exe]).returncode == 0
