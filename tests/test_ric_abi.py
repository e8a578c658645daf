"""CPU checks of the RIC boundary (include/nyx_hip_ric.h): every declared function is exported by the built library and
listed in `RIC_EXPORTS` - a list of its own, disjoint from the entries of nyx_hip.h and nyx_hip_reports.h -, the query
layout matches the ctypes mirror, bad requests are refused before any device is touched, and the C++ wrapper compiles.
No compute calls (no GPU here)."""
import ctypes as C
import os
import re

import numpy as np

from nyx_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nyx_hip_ric.h")


def _declared():
    return set(re.findall(r"^(?:int32_t|void|double|const char \*)\s*(nyx_hip_[a-z_0-9]+)\(", open(HEADER).read(), flags=re.M))


def test_every_declared_ric_function_is_exported():
    lib = _abi.load_library()
    declared = _declared()
    assert declared == {"nyx_hip_traj_ric_diff", "nyx_hip_traj_ric_diff_device", "nyx_hip_ric_sizeof"}
    assert declared == set(_abi.RIC_EXPORTS)
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in nyx_hip_ric.h but not exported"
    # they stay out of the list the Rust block is generated against, and out of the reports' list
    assert not declared & set(_abi.EXPORTS) and not declared & set(_abi.REPORT_EXPORTS)


def test_query_layout_and_constants_match_the_header():
    lib = _abi.load_library()
    header = open(HEADER).read()
    assert lib.nyx_hip_ric_sizeof(0) == C.sizeof(_abi.RicQuery) == 40
    assert lib.nyx_hip_ric_sizeof(1) == _abi.RIC_VERSION == int(re.search(r"#define NYX_HIP_RIC_VERSION (\d+)", header).group(1))
    assert lib.nyx_hip_ric_sizeof(2) == _abi.RIC_MOMENTS == int(re.search(r"#define NYX_HIP_RIC_MOMENTS (\d+)", header).group(1)) == 1 + 6 + 21
    assert lib.nyx_hip_ric_sizeof(3) == _abi.RIC_MAX_WINDOW == int(re.search(r"#define NYX_HIP_RIC_MAX_WINDOW (\d+)", header).group(1)) == 9
    assert lib.nyx_hip_ric_sizeof(99) == -1
    # field order of the mirror = field order of the header
    body = re.search(r"typedef struct nyx_hip_ric_query \{(.*?)\} nyx_hip_ric_query_t;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert names == [f for f, _ in _abi.RicQuery._fields_]


def test_bad_queries_are_refused_before_any_device_is_touched():
    """Argument validation comes first: the same answer with and without a GPU, and never a clipped request."""
    lib = _abi.load_library()
    t, one = _abi.TrajBatch(2, 4), _abi.TrajBatch(1, 4)
    ct, cone = t.as_c(), one.as_c()
    values, length, epoch0, mom = np.zeros(6 * 4 * 2), np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int64), np.zeros(4 * 28)
    vp, lp = values.ctypes.data_as(_abi.c_double_p), length.ctypes.data_as(_abi.c_int32_p)
    ep, mp = epoch0.ctypes.data_as(_abi.c_int64_p), mom.ctypes.data_as(_abi.c_double_p)
    fake_ctx = C.c_void_p(1)   # never dereferenced: every case below fails validation

    def query(step=10**9, frame_of=1, transport=1, window=5):
        q = _abi.RicQuery()
        q.step_ns, q.frame_of, q.transport, q.smooth_window = step, frame_of, transport, window
        return q

    def refused(why, ctx=fake_ctx, q=query(), n=2, ref=cone, n_ref=1, capacity=4, v=vp, l=lp, traj=ct):
        qp = C.byref(q) if q is not None else None
        rc = lib.nyx_hip_traj_ric_diff(ctx, traj, n, ref, n_ref, qp, capacity, v, l, ep, mp)
        assert rc == _abi.RC_BAD_ARG and why in _abi.last_error(), (rc, _abi.last_error())
        rc = lib.nyx_hip_traj_ric_diff_device(ctx, traj, n, ref, n_ref, qp, capacity, v, l, None, None, None)
        assert rc == _abi.RC_BAD_ARG and why in _abi.last_error(), (rc, _abi.last_error())

    refused("null ctx", ctx=None)
    refused("null query", q=None)
    refused("traj: null array", traj=None)
    refused("ref: null array", ref=None)
    refused("negative n", n=-1, n_ref=-1)
    refused("n_ref = 0", n_ref=0)
    refused("n_ref = 3", n_ref=3)
    refused("step_ns must be > 0", q=query(step=0))
    refused("step_ns must be > 0", q=query(step=-5))
    refused("capacity", capacity=0)
    refused("frame_of = 2", q=query(frame_of=2))
    refused("frame_of = -1", q=query(frame_of=-1))
    refused("transport = 2", q=query(transport=2))
    refused("smooth_window = 4", q=query(window=4))
    refused("smooth_window = 2", q=query(window=2))
    refused("smooth_window = 11", q=query(window=11))
    refused("smooth_window = -1", q=query(window=-1))
    refused("values and len arrays required", v=None)
    refused("values and len arrays required", l=None)
    assert (values == 0).all() and (length == 0).all() and (epoch0 == 0).all() and (mom == 0).all()


def test_cxx_wrapper_compiles_and_links(tmp_path):
    """include/nyx_hip_ric.hpp against the built library (host only: the layout check runs, nothing is launched)."""
    import subprocess
    _abi.load_library()
    src = tmp_path / "ric_check.cpp"
    src.write_text('#include "nyx_hip_ric.hpp"\n'
                   "nyx::RicSeries envelope(nyx::GpuPropagator &p, nyx::TrajBatch &runs, nyx::TrajBatch &nominal) {\n"
                   "    nyx::RicOptions opt;\n"
                   "    opt.moments = true;\n"
                   "    return nyx::traj_ric_diff(p, runs, nominal, 60000000000LL, 1441, opt);\n"
                   "}\n"
                   "int main() { return nyx_hip_ric_sizeof(0) == (int32_t)sizeof(nyx_hip_ric_query_t) && nyx_hip_ric_sizeof(2) == NYX_HIP_RIC_MOMENTS ? 0 : 1; }\n")
    exe = str(tmp_path / "ric_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + os.path.join(ROOT, "nyx_amd"),
                    "-lnyx_hip", "-Wl,-rpath," + os.path.join(ROOT, "nyx_amd"), "-o", exe], check=True)
    assert subprocess.run([exe]).returncode == 0
