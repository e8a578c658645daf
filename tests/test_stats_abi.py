"""CPU checks of the statistics boundary (include/nyx_hip_stats.h), after tests/test_link_abi.py: every declared function is exported
by the built library, the struct layout, the constants and the two enums match the ctypes mirror and `stats.Stat`, every refusal of
the three entries is given before a device is touched - the outputs left untouched -, a refusal of the report itself comes through
the fused entry with that report's own code and message, the Python layer refuses the same things, and a C and a C++ program that
include only the new headers compile and link.  No compute calls (no GPU here)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import nyx_amd as nx
from nyx_amd import _abi
from nyx_amd import stats as st

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nyx_hip_stats.h")


def test_every_declared_statistics_function_is_exported():
    lib = _abi.load_library()
    declared = set(re.findall(r"^(?:int32_t|void|double|const char \*)\s*(nyx_hip_[a-z_0-9]+)\(", open(HEADER).read(), flags=re.M))
    assert declared == {"nyx_hip_series_stats", "nyx_hip_series_stats_device", "nyx_hip_traj_series_stats", "nyx_hip_stats_sizeof"} == set(_abi.STATS_EXPORTS)
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in nyx_hip_stats.h but not exported"
        assert _abi.stats_entry(lib, name) is getattr(lib, name)
    others = (_abi.EXPORTS, _abi.REPORT_EXPORTS, _abi.RIC_EXPORTS, _abi.GROUNDTRACK_EXPORTS, _abi.AER_EXPORTS, _abi.ECLIPSE_EXPORTS, _abi.FRAME_EXPORTS,
              _abi.LINK_EXPORTS)
    assert not [n for names in others for n in names if n in declared]
    # nyx_hip.h does not know them: NYX_HIP_ABI_VERSION and its declaration list are unchanged
    main = open(os.path.join(ROOT, "include", "nyx_hip.h")).read()
    assert "nyx_hip_stats" not in main and "series_stats" not in main and "NYX_HIP_STAT" not in main
    assert len(lib.nyx_hip_series_stats.argtypes) == 9 and len(lib.nyx_hip_series_stats_device.argtypes) == 10 and len(lib.nyx_hip_traj_series_stats.argtypes) == 14


def test_an_older_library_gives_a_clear_error():
    class Old:   # a library built before the statistics: no such symbol
        pass

    with pytest.raises(RuntimeError, match="has no nyx_hip_series_stats.*rebuild"):
        _abi.stats_entry(Old())
    with pytest.raises(RuntimeError, match="has no nyx_hip_traj_series_stats.*rebuild"):
        _abi.stats_entry(Old(), "nyx_hip_traj_series_stats")


def test_layout_constants_and_enums_match_the_header():
    lib = _abi.load_library()
    header = open(HEADER).read()
    assert lib.nyx_hip_stats_sizeof(0) == C.sizeof(_abi.StatsQuery) == 4 + 4 + 8 * 8 == 72
    assert lib.nyx_hip_stats_sizeof(1) == _abi.STATS_VERSION == int(re.search(r"#define NYX_HIP_STATS_VERSION (\d+)", header).group(1)) == 1
    assert lib.nyx_hip_stats_sizeof(2) == _abi.STAT_FIXED == st.STAT_FIXED == int(re.search(r"#define NYX_HIP_STAT_FIXED (\d+)", header).group(1)) == 10
    assert lib.nyx_hip_stats_sizeof(3) == _abi.MAX_STAT_PROBS == st.MAX_STAT_PROBS == int(re.search(r"#define NYX_HIP_MAX_STAT_PROBS (\d+)", header).group(1)) == 8
    assert lib.nyx_hip_stats_sizeof(4) == _abi.SERIES_COUNT == 7 and lib.nyx_hip_stats_sizeof(5) == -1 and lib.nyx_hip_stats_sizeof(-1) == -1
    assert [(f, getattr(_abi.StatsQuery, f).offset) for f, _ in _abi.StatsQuery._fields_] == [("n_probs", 0), ("reserved", 4), ("prob", 8)]
    # the values of the two enums are part of the ABI: never renumbered
    stat = {k: int(v) for k, v in re.findall(r"NYX_HIP_STAT_([A-Z]+) = (\d+)", header)}
    assert stat == {"HELD": 0, "COUNT": 1, "MIN": 2, "MAX": 3, "ARGMIN": 4, "ARGMAX": 5, "FINITE": 6, "SHIFT": 7, "SUM": 8, "SUMSQ": 9} == {s.name: int(s) for s in st.Stat}
    kind = {k: int(v) for k, v in re.findall(r"NYX_HIP_SERIES_([A-Z_]+) = (\d+)", header)}
    assert kind == {"VALUES": 0, "GROUND_TRACK": 1, "AER": 2, "ECLIPSE": 3, "FRAME": 4, "LINK": 5, "RIC": 6, "COUNT": 7}
    assert [_abi.SERIES_VALUES, _abi.SERIES_GROUND_TRACK, _abi.SERIES_AER, _abi.SERIES_ECLIPSE, _abi.SERIES_FRAME, _abi.SERIES_LINK, _abi.SERIES_RIC] == list(range(7))
    assert _abi.SERIES_KINDS == {"traj_values": 0, "traj_ground_track": 1, "traj_aer": 2, "traj_eclipse": 3, "traj_frame_values": 4, "traj_link": 5, "traj_ric_diff": 6}
    # the header states the choice for the kernel time, the NaN it writes and what is out of scope
    flat = " ".join(header.replace("\n *", "\n").split())
    for words in ("the time of the REDUCER's launch alone", "0x7FF8000000000000", "quantiles do not all-reduce", "n == 0 is not an error", "-0.0 before +0.0"):
        assert words in flat, words
    # STAT_LDS_KEYS is a named constant of the kernel's arguments, and 10 000 runs fit
    args = open(os.path.join(ROOT, "nyx_amd", "csrc", "stats_args.h")).read()
    assert int(re.search(r"#define STAT_LDS_KEYS (\d+)", args).group(1)) * 8 + 2048 <= 160 * 1024 and int(re.search(r"#define STAT_LDS_KEYS (\d+)", args).group(1)) >= 10000


def _block():
    values, length, out = np.zeros(2 * 3 * 4), np.full(4, 3, dtype=np.int32), np.full(2 * 3 * 18, 12345.0)
    return values, length, out, values.ctypes.data_as(_abi.c_double_p), length.ctypes.data_as(_abi.c_int32_p), out.ctypes.data_as(_abi.c_double_p)


def test_bad_blocks_are_refused_before_any_device_is_touched():
    lib = _abi.load_library()
    values, length, out, vp, lp, op = _block()
    fake_ctx = C.c_void_p(1)   # never dereferenced: every case below fails on the arguments alone
    nan = float("nan")

    def query(probs=(0.5,), n_probs=None):
        q = _abi.StatsQuery()
        q.n_probs = len(probs) if n_probs is None else n_probs
        q.prob[:len(probs)] = probs
        return q

    def refused(ctx, q, why, v=vp, l=lp, o=op, rows=2, cap=3, n=4):
        qp = C.byref(q) if q is not None else None
        rc = lib.nyx_hip_series_stats(ctx, v, l, None, rows, cap, n, qp, o)
        assert rc == _abi.RC_BAD_ARG and why in _abi.last_error(), (rc, _abi.last_error())
        rc = lib.nyx_hip_series_stats_device(ctx, v, l, None, rows, cap, n, qp, o, None)
        assert rc == _abi.RC_BAD_ARG and why in _abi.last_error(), (rc, _abi.last_error())

    refused(None, query(), "null ctx")
    refused(fake_ctx, None, "series_stats: null statistics query")
    refused(fake_ctx, query(n_probs=-1), "n_probs = -1, 0 .. 8")
    refused(fake_ctx, query(n_probs=9), "n_probs = 9, 0 .. 8")
    for bad in (nan, -1e-9, 1.0 + 1e-9, float("inf")):
        refused(fake_ctx, query((0.5, bad)), "prob[1] must lie in [0, 1]")
    refused(fake_ctx, query(), "n_rows must be >= 1", rows=0)
    refused(fake_ctx, query(), "capacity must be 1 .. 2^31 - 1", cap=0)
    refused(fake_ctx, query(), "capacity must be 1 .. 2^31 - 1", cap=2**31)
    refused(fake_ctx, query(), "n must be 0 .. 2^31 - 1", n=-1)
    refused(fake_ctx, query(), "n must be 0 .. 2^31 - 1", n=2**31)
    refused(fake_ctx, query(), "stats array required", o=None)
    refused(fake_ctx, query(), "values and len arrays required", v=None)
    refused(fake_ctx, query(), "values and len arrays required", l=None)
    assert (out == 12345.0).all()


def test_the_fused_entry_refuses_its_own_then_the_reports():
    lib = _abi.load_library()
    _, length, out, _, lp, op = _block()
    t = _abi.TrajBatch(4, 4)
    ct = t.as_c()
    fake_ctx = C.c_void_p(1)
    sq = _abi.stats_query((0.01, 0.5, 0.99))
    queries = {_abi.SERIES_VALUES: _abi.ValuesQuery, _abi.SERIES_GROUND_TRACK: _abi.GtQuery, _abi.SERIES_AER: _abi.AerQuery, _abi.SERIES_ECLIPSE: _abi.EclQuery,
               _abi.SERIES_FRAME: _abi.FrameQuery, _abi.SERIES_LINK: _abi.LinkQuery, _abi.SERIES_RIC: _abi.RicQuery}

    def refused(why, ctx=fake_ctx, kind=_abi.SERIES_VALUES, traj=ct, ref=None, n_ref=0, q=None, size=None, cap=3, stats_q=sq, o=op, l=lp, rc_want=_abi.RC_BAD_ARG):
        q = queries.get(kind, _abi.ValuesQuery)() if q is None else q
        rc = lib.nyx_hip_traj_series_stats(ctx, kind, C.byref(traj) if traj is not None else None, 4, C.byref(ref) if ref is not None else None, n_ref,
                                           C.byref(q) if q is not False else None, C.sizeof(q) if size is None else size, cap, None,
                                           C.byref(stats_q) if stats_q is not None else None, o, l, None)
        assert rc == rc_want and why in _abi.last_error(), (rc, _abi.last_error())

    refused("null ctx", ctx=None)
    refused("kind = 7 is not a nyx_hip_series_kind", kind=7)
    refused("kind = -1 is not a nyx_hip_series_kind", kind=-1)
    refused("null traj", traj=None)
    for kind, cls in queries.items():   # the guard of the void pointer: the library's own size of that kind's query
        with_ref = kind in (_abi.SERIES_LINK, _abi.SERIES_RIC)
        name = [k for k, v in _abi.SERIES_KINDS.items() if v == kind][0]
        refused(f"query_size = {C.sizeof(cls) + 4}, the query of {name} is {C.sizeof(cls)} bytes", kind=kind, size=C.sizeof(cls) + 4, ref=ct if with_ref else None, n_ref=1)
        refused("query_size = 0", kind=kind, size=0)
        if with_ref:
            refused(f"{name} needs a second batch (ref)", kind=kind)
        else:
            refused(f"{name} takes no second batch (ref)", kind=kind, ref=ct, n_ref=1)
    refused("null statistics query", stats_q=None)
    bad = _abi.StatsQuery()
    bad.n_probs, bad.prob[0] = 1, 1.5
    refused("prob[0] must lie in [0, 1]", stats_q=bad)
    bad.n_probs = 9
    refused("n_probs = 9", stats_q=bad)
    refused("stats and len arrays required", o=None)
    refused("stats and len arrays required", l=None)
    # behind them the report's own refusals, code and message unchanged: the same check functions
    q = _abi.ValuesQuery()
    q.n_params, q.step_ns = 0, 10**9
    refused("traj_values: n_params = 0, 1 .. 8 parameters per call", q=q)
    q.n_params, q.step_ns = 1, 0
    refused("traj_values: step_ns must be > 0", q=q)
    q.step_ns = 10**9
    refused("traj_values: capacity must be 1 .. 2^31 - 1", q=q, cap=0)
    rq = _abi.RicQuery()
    rq.step_ns, rq.smooth_window = 10**9, 4
    refused("traj_ric_diff: smooth_window = 4", kind=_abi.SERIES_RIC, q=rq, ref=ct, n_ref=1)
    rq.smooth_window = 5
    refused("traj_ric_diff: n_ref = 3", kind=_abi.SERIES_RIC, q=rq, ref=ct, n_ref=3)
    aq = _abi.AerQuery()
    aq.n_params, aq.step_ns, aq.n_stations = 1, 10**9, 0
    refused("traj_aer: n_stations = 0", kind=_abi.SERIES_AER, q=aq)
    assert (out == 12345.0).all() and (length == 3).all()


def test_the_python_layer_refuses_the_same_things():
    for bad in ((1.5,), (-0.1,), (float("nan"),), tuple([0.5] * 9)):
        with pytest.raises(ValueError, match="prob|n_probs"):
            _abi.stats_query(bad)
        with pytest.raises(ValueError):
            st.check_probs(bad)
    q = _abi.stats_query((0.0, 1.0))
    assert q.n_probs == 2 and list(q.prob)[:2] == [0.0, 1.0]
    assert st.request((0.5,)) == st.Request((0.5,), None) and st.request(st.Request((0.5,), [0, 1])).status == [0, 1]
    res = nx.Results([], "none")
    with pytest.raises(ValueError, match="report must be one of"):
        res.series_stats("final_rv")
    with pytest.raises(ValueError, match="probabilit"):
        res.series_stats("values_of", [nx.StateParameter.X], 10**9, probs=(2.0,))
    with pytest.raises(ValueError, match="carry no trajectories"):
        res.series_stats("values_of", [nx.StateParameter.X], 10**9, probs=(0.5,))


def test_c_and_cxx_programs_compile_and_link(tmp_path):
    """include/nyx_hip_stats.h from C, include/nyx_hip_stats.hpp from C++: syntax alone, then against the built library (host only:
    the layout check and a refusal run, nothing is launched)."""
    _abi.load_library()
    inc = "-I" + os.path.join(ROOT, "include")
    link = ["-L" + os.path.join(ROOT, "nyx_amd"), "-lnyx_hip", "-Wl,-rpath," + os.path.join(ROOT, "nyx_amd")]
    c_src = tmp_path / "stats_check.c"
    c_src.write_text('#include "nyx_hip_stats.h"\n'
                     "int main(void) { nyx_hip_stats_query_t q; double out[10]; q.n_probs = 9; q.reserved = 0;\n"
                     "    if (nyx_hip_series_stats(0, 0, 0, 0, 1, 1, 0, &q, out) != NYX_HIP_RC_BAD_ARG) return 2;\n"
                     "    return nyx_hip_stats_sizeof(0) == (int32_t)sizeof(nyx_hip_stats_query_t) && nyx_hip_stats_sizeof(2) == NYX_HIP_STAT_FIXED &&\n"
                     "           NYX_HIP_STAT_SUMSQ == 9 && NYX_HIP_SERIES_RIC == 6 && nyx_hip_stats_sizeof(1) == NYX_HIP_STATS_VERSION ? 0 : 1; }\n")
    exe = str(tmp_path / "stats_check_c")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", inc, str(c_src), *link, "-o", exe], check=True)
    assert subprocess.run([exe]).returncode == 0
    src = tmp_path / "stats_check.cpp"
    src.write_text('#include "nyx_hip_reports.h"\n#include "nyx_hip_stats.hpp"\n'
                   "nyx::SeriesStats band(nyx::GpuPropagator &p, nyx::TrajBatch &runs, const nyx_hip_values_query_t &q) {\n"
                   "    return nyx::traj_series_stats(p, NYX_HIP_SERIES_VALUES, runs, nullptr, q, q.n_params, 91, {0.01, 0.5, 0.99});\n"
                   "}\n"
                   "nyx::SeriesStats block(nyx::GpuPropagator &p, const std::vector<double> &v, const std::vector<int32_t> &len) {\n"
                   "    return nyx::series_stats(p, v.data(), len.data(), nullptr, 1, 1, (int64_t)len.size(), {0.5});\n"
                   "}\n"
                   "int main() { return nyx_hip_stats_sizeof(0) == (int32_t)sizeof(nyx_hip_stats_query_t) && nyx_hip_stats_sizeof(3) == NYX_HIP_MAX_STAT_PROBS &&\n"
                   "             nyx_hip_stats_sizeof(4) == NYX_HIP_SERIES_COUNT && nyx::stats_query({0.5}).n_probs == 1 ? 0 : 1; }\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", inc, str(src)], check=True)
    exe = str(tmp_path / "stats_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", inc, str(src), *link, "-o", exe], check=True)
    assert subprocess.run([exe]).returncode == 0
