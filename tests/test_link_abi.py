"""CPU checks of the link boundary (include/nyx_hip_link.h), the twin of tests/test_frame_abi.py: every declared function is exported by
the built library, the struct layout and the parameter codes match the ctypes mirror and `LinkParameter`, every refusal that can be
told from the query alone is given before a device is touched - by both flavours, the outputs left untouched -, the Python layer
refuses what the device path refuses, and a C and a C++ program that include only the new headers compile and link.  No compute calls
(no GPU here).  What a query asks OF THE CONTEXT - a segment index beyond the context's segments, the integration-frame swap refused
with NYX_HIP_RC_UNSUPPORTED - needs a context, which needs a device: the rule itself (`check_link_context` of csrc/series_host.h,
chained behind `check_link_series` exactly as abi.cpp chains them) is run, with every refusal and its message, by the stand-alone
program of tests/test_link_host_cxx.py (tests/cxx/link_host_check.cpp); here the source of abi.cpp is held to that chaining."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import nyx_amd as nx
from nyx_amd import _abi, links
from nyx_amd.links import LinkParameter as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nyx_hip_link.h")


def _declared():
    return set(re.findall(r"^(?:int32_t|void|double|const char \*)\s*(nyx_hip_[a-z_0-9]+)\(", open(HEADER).read(), flags=re.M))


def _fields(header, struct):
    body = re.search(r"typedef struct %s \{(.*?)\} %s_t;" % (struct, struct), header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [re.sub(r"\[.*", "", n.strip()) for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]


def test_every_declared_link_function_is_exported():
    lib = _abi.load_library()
    declared = _declared()
    assert declared == {"nyx_hip_traj_link", "nyx_hip_traj_link_device", "nyx_hip_link_sizeof"}
    assert declared == set(_abi.LINK_EXPORTS)
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in nyx_hip_link.h but not exported"
        assert _abi.link_entry(lib, name) is getattr(lib, name)
    # the entries stay out of the lists of the other headers (the Rust block is generated against EXPORTS)
    assert not declared & (set(_abi.EXPORTS) | set(_abi.REPORT_EXPORTS) | set(_abi.RIC_EXPORTS) | set(_abi.GROUNDTRACK_EXPORTS) | set(_abi.AER_EXPORTS)
                           | set(_abi.ECLIPSE_EXPORTS) | set(_abi.FRAME_EXPORTS))
    # and nyx_hip.h does not know them: NYX_HIP_ABI_VERSION and its declaration list are unchanged
    main = open(os.path.join(ROOT, "include", "nyx_hip.h")).read()
    assert "nyx_hip_link" not in main and "nyx_hip_traj_link" not in main and "NYX_HIP_LNK" not in main
    # registered from the table of the parameter series, with the second batch and the first epochs in its signature
    assert "link" in _abi.SERIES_ENTRIES and _abi.SERIES_ENTRIES["link"][:2] == ("link", _abi.LinkQuery) and "link" in _abi.REF_SERIES
    assert len(lib.nyx_hip_traj_link.argtypes) == 10 and len(lib.nyx_hip_traj_link_device.argtypes) == 11
    assert len(lib.nyx_hip_traj_frame_values.argtypes) == 7 and len(lib.nyx_hip_traj_frame_values_device.argtypes) == 8   # (the others as they were)


def test_an_older_library_gives_a_clear_error():
    class Old:   # a library built before the link report: no such symbol
        pass

    with pytest.raises(RuntimeError, match="has no nyx_hip_traj_link.*rebuild"):
        _abi.link_entry(Old())


def test_query_layout_and_constants_match_the_header():
    lib = _abi.load_library()
    header = open(HEADER).read()
    assert C.sizeof(_abi.EclBody) == 48
    assert lib.nyx_hip_link_sizeof(0) == C.sizeof(_abi.LinkQuery) == 4 + 32 + 32 + 4 + 3 * 8 + 4 + 4 + 8 * 48 == 488
    assert lib.nyx_hip_link_sizeof(1) == _abi.LINK_VERSION == int(re.search(r"#define NYX_HIP_LINK_VERSION (\d+)", header).group(1))
    assert lib.nyx_hip_link_sizeof(3) == _abi.MAX_LINK_PARAMS == int(re.search(r"#define NYX_HIP_MAX_LINK_PARAMS (\d+)", header).group(1)) == 8
    assert lib.nyx_hip_link_sizeof(4) == _abi.MAX_LINK_BODIES == int(re.search(r"#define NYX_HIP_MAX_LINK_BODIES (\d+)", header).group(1)) == 8 == links.MAX_BODIES
    assert lib.nyx_hip_link_sizeof(5) == -1 and lib.nyx_hip_link_sizeof(-1) == -1
    # field order of the mirror = field order of the header
    assert _fields(header, "nyx_hip_link_query") == [f for f, _ in _abi.LinkQuery._fields_]
    assert [getattr(_abi.LinkQuery, f).offset for f in ("n_params", "param", "param_body", "has_window", "step_ns", "start_ns", "end_ns", "n_bodies", "_pad",
                                                        "bodies")] == [0, 4, 36, 68, 72, 80, 88, 96, 100, 104]
    assert '#include "nyx_hip_eclipse.h"' in header and "nyx_hip_ecl_body_t bodies[NYX_HIP_MAX_LINK_BODIES]" in header
    assert _abi.MAX_CHAIN == links.MAX_CHAIN
    # the header says what is restated and unpinned, what the reference's Doppler is, and what is out of scope
    flat = " ".join(header.replace("\n *", "\n").split())
    for words in ("Vallado's SIGHT test", "parity-unpinned", "despite the comment beside it", "COINCIDENT SPACECRAFT", "Not guarded",
                  "light time, aberration, measurement noise, the integration-time average", "antenna masks"):
        assert words in flat, words


def test_parameter_codes_match_the_header_and_cover_the_enum():
    lib = _abi.load_library()
    header = open(HEADER).read()
    enum = dict((k, int(v)) for k, v in re.findall(r"NYX_HIP_LNK_([A-Z_0-9]+) = (\d+)", header))
    count = enum.pop("COUNT")
    assert count == 12 == lib.nyx_hip_link_sizeof(2) == _abi.LINK_COUNT == len(L) == len(_abi.LINK_PARAM)
    assert sorted(enum.values()) == list(range(12))
    names = {"Range": "RANGE", "RangeRate": "RANGE_RATE", "ReferenceDoppler": "REFERENCE_DOPPLER", "Visible": "VISIBLE", "ObstructingBody": "OBSTRUCTING_BODY",
             "Clearance": "CLEARANCE", "RelativeSpeed": "RELATIVE_SPEED", "LosX": "LOS_X", "LosY": "LOS_Y", "LosZ": "LOS_Z", "BodyClearance": "BODY_CLEARANCE",
             "BodyObstructs": "BODY_OBSTRUCTS"}
    assert {names[name]: code for name, code in _abi.LINK_PARAM.items()} == enum
    assert {p.name: int(p) for p in L} == _abi.LINK_PARAM
    assert _abi.LINK_PARAM == {"Range": 0, "RangeRate": 1, "ReferenceDoppler": 2, "Visible": 3, "ObstructingBody": 4, "Clearance": 5, "RelativeSpeed": 6,
                               "LosX": 7, "LosY": 8, "LosZ": 9, "BodyClearance": 10, "BodyObstructs": 11}                # never renumbered
    assert {int(p) for p in links.PER_BODY} == set(range(_abi.LINK_FIRST_PER_BODY, 12))


def test_bad_queries_are_refused_before_any_device_is_touched():
    """Argument validation comes first: the same answer with and without a GPU, and never a clipped request."""
    lib = _abi.load_library()
    t = _abi.TrajBatch(2, 4)
    ct = t.as_c()
    values, length, epoch0 = np.zeros(8 * 4 * 2), np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int64)
    vp, lp, ep = values.ctypes.data_as(_abi.c_double_p), length.ctypes.data_as(_abi.c_int32_p), epoch0.ctypes.data_as(_abi.c_int64_p)
    fake_ctx = C.c_void_p(1)   # never dereferenced: every case below fails on the query alone
    nan, inf = float("nan"), float("inf")

    def query(n_params=1, param=int(L.Range), step=10**9, n_bodies=2, n_chain=2, radius=1737.4, segment=None, sign=None, param_body=0):
        q = _abi.LinkQuery()
        q.n_params, q.step_ns, q.n_bodies = n_params, step, n_bodies
        for k in range(8):
            q.param[k], q.param_body[k] = param, param_body
        q.bodies[0].n_chain, q.bodies[0].mean_radius_km = 0, 6378.14
        q.bodies[1].n_chain, q.bodies[1].mean_radius_km = n_chain, radius
        for k, (seg, sg) in enumerate([(3, 1), (0, -1), (1, 1), (2, 1)]):
            q.bodies[1].chain_segment[k], q.bodies[1].chain_sign[k] = seg, sg
        if segment:
            q.bodies[1].chain_segment[segment[0]] = segment[1]
        if sign:
            q.bodies[1].chain_sign[sign[0]] = sign[1]
        return q

    def refused(ctx, q, capacity, v, l, why, n=2, ref=ct, n_ref=1):
        qp, rp = (C.byref(q) if q is not None else None), (C.byref(ref) if ref is not None else None)
        rc = lib.nyx_hip_traj_link(ctx, C.byref(ct), n, rp, n_ref, qp, capacity, v, l, ep)
        assert rc == _abi.RC_BAD_ARG and why in _abi.last_error(), (rc, _abi.last_error())
        rc = lib.nyx_hip_traj_link_device(ctx, C.byref(ct), n, rp, n_ref, qp, capacity, v, l, None, None)
        assert rc == _abi.RC_BAD_ARG and why in _abi.last_error(), (rc, _abi.last_error())

    refused(None, query(), 4, vp, lp, "null ctx")
    refused(fake_ctx, query(), 4, vp, lp, "ref: null array", ref=None)
    refused(fake_ctx, None, 4, vp, lp, "traj_link: null query")
    refused(fake_ctx, query(), 4, vp, lp, "negative n", n=-1, n_ref=-1)
    refused(fake_ctx, query(), 4, vp, lp, "n_ref = 3, one transmitter trajectory or one per run (n = 2)", n_ref=3)
    refused(fake_ctx, query(), 4, vp, lp, "n_ref = 0", n_ref=0)
    refused(fake_ctx, query(n_params=0), 4, vp, lp, "n_params = 0")
    refused(fake_ctx, query(n_params=9), 4, vp, lp, "n_params = 9")
    refused(fake_ctx, query(param=12), 4, vp, lp, "param[0] = 12 is not a nyx_hip_link_param")
    refused(fake_ctx, query(param=-1), 4, vp, lp, "param[0] = -1")
    refused(fake_ctx, query(step=0), 4, vp, lp, "step_ns must be > 0")
    refused(fake_ctx, query(step=-5), 4, vp, lp, "step_ns must be > 0")
    refused(fake_ctx, query(), 0, vp, lp, "capacity")
    refused(fake_ctx, query(), 4, None, lp, "values and len arrays required")
    refused(fake_ctx, query(), 4, vp, None, "values and len arrays required")
    refused(fake_ctx, query(n_bodies=-1), 4, vp, lp, "n_bodies = -1, 0 .. 8")
    refused(fake_ctx, query(n_bodies=9), 4, vp, lp, "n_bodies = 9, 0 .. 8")
    refused(fake_ctx, query(n_chain=-1), 4, vp, lp, "bodies[1].n_chain = -1, 0 .. 4")
    refused(fake_ctx, query(n_chain=5), 4, vp, lp, "bodies[1].n_chain = 5, 0 .. 4")
    refused(fake_ctx, query(segment=(1, -1)), 4, vp, lp, "bodies[1].chain_segment[1] = -1")
    refused(fake_ctx, query(sign=(0, 0)), 4, vp, lp, "bodies[1].chain_sign[0] = 0, +1 or -1")
    refused(fake_ctx, query(n_chain=4, sign=(3, 2)), 4, vp, lp, "bodies[1].chain_sign[3] = 2")
    for radius in (0.0, -1.0, nan, inf):
        refused(fake_ctx, query(radius=radius), 4, vp, lp, "bodies[1].mean_radius_km must be finite and > 0")
    refused(fake_ctx, query(param=int(L.BodyClearance), param_body=2), 4, vp, lp, "param_body[0] = 2, param[0] is a per-body parameter of bodies[0 .. 1]")
    refused(fake_ctx, query(param=int(L.BodyObstructs), param_body=-1), 4, vp, lp, "param_body[0] = -1")
    refused(fake_ctx, query(param=int(L.BodyObstructs), n_bodies=0), 4, vp, lp, "per-body parameter and the query names no body")
    assert (values == 0).all() and (length == 0).all() and (epoch0 == 0).all()


def test_the_context_is_asked_behind_the_query_alone():
    """abi.cpp chains check_link_series (never reads the context) and check_link_context (its segments, no frame swap), in that order,
    in front of everything that touches a device - in both flavours."""
    src = open(os.path.join(ROOT, "nyx_amd", "csrc", "abi.cpp")).read()
    body = src[src.index("static Refusal check_link("):]
    body = body[:body.index("\n}\n")]
    assert body.index("check_link_series(ctx, traj, n, ref, n_ref, q, capacity, values, len)") < body.index("check_link_context(*q, ctx->host_cfg.n_seg, ctx->swap_n_chain != 0)")
    for entry in ("nyx_hip_traj_link_device", "nyx_hip_traj_link"):
        fn = src[src.index(f'extern "C" int32_t {entry}('):]
        fn = fn[fn.index("{") + 1:fn.index("\n}\n")]
        assert fn.lstrip().startswith("if (Refusal r = check_link(ctx, traj, n, ref, n_ref, q, capacity, values, len)) return refused(r);"), entry
    host = open(os.path.join(ROOT, "nyx_amd", "csrc", "series_host.h")).read()
    assert "NYX_HIP_RC_UNSUPPORTED" in host[host.index("inline Refusal check_link_context("):host.index("// ---- the one output block")]
    # the host flavour goes through the staging and the one output block of the RIC report: values + epoch0 + len
    fn = src[src.index('extern "C" int32_t nyx_hip_traj_link('):]
    assert "series_host(ctx, traj, n, ref, n_ref, q->n_params, capacity, {values, len, epoch0_ns, nullptr}" in fn[:fn.index("\n}\n")]


def test_the_python_layer_refuses_what_the_device_path_refuses():
    class Ctx:   # no almanac, no centre
        compiled = None

    earth = nx.Frame(nx.EARTH, 398600.4, 6378.14)

    class Compiled:
        almanac, central = None, earth

    class Centred:
        compiled = Compiled()

    one = _abi.TrajBatch(1, 2)
    res = nx.Results([], "none", _traj_ctx=Ctx(), _traj_batch=_abi.TrajBatch(1, 2))
    with pytest.raises(ValueError, match="a positive step"):
        res.link_views(one, 0)
    with pytest.raises(ValueError, match="at least one parameter"):
        res.link_views(one, 10**9, params=[])
    with pytest.raises(ValueError, match="does not know the central frame"):
        res.link_views(one, 10**9)
    with pytest.raises(ValueError, match="a window needs both"):
        res.link_views(one, 10**9, start_ns=5)
    res = nx.Results([], "none", _traj_ctx=Centred(), _traj_batch=_abi.TrajBatch(1, 2))
    with pytest.raises(TypeError, match="not a LinkParameter"):
        res.link_views(one, 10**9, params=[nx.StateParameter.Rmag])
    with pytest.raises(ValueError, match="needs an almanac"):
        res.link_views(one, 10**9, bodies=[earth, nx.Frame(nx.MOON, 4902.8, 1737.4)])
    with pytest.raises(ValueError, match="per-body parameter"):
        res.link_views(one, 10**9, params=[L.BodyClearance])
    with pytest.raises(ValueError, match="one transmitter trajectory"):
        res.link_views(_abi.TrajBatch(2, 2), 10**9)
    with pytest.raises(ValueError, match="carry no trajectories"):
        nx.Results([], "none", _traj_ctx=Centred()).link_views(one, 10**9)
    series = nx.LinkSeries([earth], [L.RangeRate], np.zeros((1, 0, 2)), np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int64), 10**9, np.ones(2, dtype=bool))
    with pytest.raises(ValueError, match="does not hold Range"):
        series.closest_range()
    with pytest.raises(ValueError, match="holds none of"):
        series.visible_fraction()


def test_c_and_cxx_programs_compile_and_link(tmp_path):
    """include/nyx_hip_link.h from C, include/nyx_hip_link.hpp from C++: syntax alone, then against the built library (host only: the
    layout check runs, nothing is launched)."""
    _abi.load_library()
    inc = "-I" + os.path.join(ROOT, "include")
    link = ["-L" + os.path.join(ROOT, "nyx_amd"), "-lnyx_hip", "-Wl,-rpath," + os.path.join(ROOT, "nyx_amd")]
    c_src = tmp_path / "lnk_check.c"
    c_src.write_text('#include "nyx_hip_link.h"\n'
                     "int main(void) { nyx_hip_link_query_t q; q.n_bodies = 0; (void)q;\n"
                     "    return nyx_hip_link_sizeof(0) == (int32_t)sizeof(nyx_hip_link_query_t) && nyx_hip_link_sizeof(2) == NYX_HIP_LNK_COUNT &&\n"
                     "           NYX_HIP_LNK_BODY_OBSTRUCTS == 11 && nyx_hip_link_sizeof(1) == NYX_HIP_LINK_VERSION ? 0 : 1; }\n")
    exe = str(tmp_path / "lnk_check_c")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", inc, str(c_src), *link, "-o", exe], check=True)
    assert subprocess.run([exe]).returncode == 0
    src = tmp_path / "lnk_check.cpp"
    src.write_text('#include "nyx_hip_link.hpp"\n'
                   "nyx::LinkSeries relay(nyx::GpuPropagator &p, nyx::TrajBatch &runs, nyx::TrajBatch &tx) {\n"
                   "    nyx::LinkBody earth;\n"
                   "    earth.mean_radius_km = 6378.14;\n"
                   "    return nyx::traj_link(p, runs, tx, {earth}, {{NYX_HIP_LNK_RANGE, 0}, {NYX_HIP_LNK_VISIBLE, 0}, {NYX_HIP_LNK_BODY_CLEARANCE, 0}},\n"
                   "                          60000000000LL, 91);\n"
                   "}\n"
                   "int main() { return nyx_hip_link_sizeof(0) == (int32_t)sizeof(nyx_hip_link_query_t) && NYX_HIP_LNK_COUNT == 12 &&\n"
                   "             nyx_hip_link_sizeof(3) == NYX_HIP_MAX_LINK_PARAMS && nyx_hip_link_sizeof(4) == NYX_HIP_MAX_LINK_BODIES ? 0 : 1; }\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", inc, str(src)], check=True)
    exe = str(tmp_path / "lnk_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", inc, str(src), *link, "-o", exe], check=True)
    assert subprocess.run([exe]).returncode == 0
