"""Builders for the ephemeris-table tests (host logic only): four almanacs that hold the SAME leading records and land in the four
combinations of record layout (sixteen wide / packed) and placement (LDS / global memory) nyx_amd/csrc/ctx_build.h knows, and a
batch whose lanes sit on different records and cross record seams.

    name  layout  placement  span [d]  records  packed    padded     (doubles; the context adds a 16-double tail)
    A     padded  LDS           40        47      1 852     2 350    the table of every other GPU test
    B     packed  LDS           64        61      2 420     3 050
    C     padded  global       400       282     11 190    14 100
    D     packed  global    32 768    21 523    854 768 1 076 150    (padded above 2^20 doubles = 8 MiB)

The sizes that decide, for the plain kernels (restated from pk_state_lds.h / ctx_build.h and checked against the library's own
`nyx_kernel_lds_bytes` in tests/test_ephem_table_cases.py): the records go into LDS when they are at most 24 KiB = 3 072 doubles AND
the workgroup layout with them is at most 160 KiB, which leaves 2 560 doubles beside the plain kernel's buffers (3 136 beside the quad
STM layout, 1 216 beside the D3 one).  So B is the table whose packed form (2 436 with the tail) fits and whose padded form (3 066)
does not - the 72-day table (2 686 packed) would not fit either way.

A, B and C are `ephem.build_almanac` itself: its start is aligned to 32 days whatever the span and every record is fitted on its own,
so a longer span only appends records.  D would take a minute that way (21 523 fits); its first records are C's - fitted - and the
rest are NEVER-VISITED copies of each segment's last fitted record with the midpoint advanced (the second of the two ways the table
may be made quickly: no run of these tests leaves the first 40 days, and a copy keeps the leading records bit for bit, which one
solve over all records - another LAPACK call, another order of operations - would not promise)."""
import ctypes as C

import numpy as np

import nyx_amd as nx
from nyx_amd import _abi, ephem
from scenarios import EPOCH0_NS, dispersed_leo_batch

DAY = 86400.0
SPAN_DAYS = {"A": 40.0, "B": 64.0, "C": 400.0, "D": 32768.0}
LAYOUT = {"A": "padded", "B": "packed", "C": "padded", "D": "packed"}      # for the PLAIN kernels (an STM context decides beside D3)
IN_LDS = {"A": 1, "B": 1, "C": 0, "D": 0}
TAIL = 16                                   # doubles behind the records (ctx_build.h: the 16-wide coefficient window)
REC_LDS_MAX = 24 * 1024 // 8                # kRecordsLdsMax in doubles
PAD16_MAX = (8 << 20) // 8                  # the padded table may take 8 MiB at most
KERNEL_LDS_MAX = 160 * 1024                 # kKernelLdsMax
PLAIN, D3, QUAD = 0, 1, 2                   # `stm` of nyx_kernel_lds_bytes
_CACHE = {}


def extend_segment(s: nx.ChebySegment, n: int) -> nx.ChebySegment:
    """`s` continued to `n` records: the new ones copies of its last record with their own midpoints."""
    have = s.records.shape[0]
    assert n >= have
    recs = np.empty((n, s.records.shape[1]))
    recs[:have] = s.records
    recs[have:] = s.records[-1]
    recs[have:, 0] = s.init_et_s + (np.arange(have, n) + 0.5) * s.interval_s
    return nx.ChebySegment(s.init_et_s, s.interval_s, recs)


def extended(base: nx.Almanac, et0_s: float, span_days: float) -> nx.Almanac:
    """`base` with every segment continued to `et0 + span`: the record count `ephem.build_almanac` gives that span."""
    out = nx.Almanac()
    end = et0_s + span_days * DAY
    for s in base.segments:
        out.add_segment(extend_segment(s, int(np.ceil((end - s.init_et_s) / s.interval_s))))
    for naif, b in base.bodies.items():
        out.add_body(naif, b["mu"], b["radius"], b["chain"])
    return out


def almanac(name: str) -> nx.Almanac:
    """The almanac A, B, C or D (built once)."""
    if name not in _CACHE:
        et0 = nx.to_seconds(EPOCH0_NS)
        if name == "D":
            _CACHE[name] = extended(almanac("C"), et0, SPAN_DAYS["D"])
        else:
            _CACHE[name] = ephem.build_almanac(et0, SPAN_DAYS[name])
    return _CACHE[name]


def table_sizes(segments):
    """(packed, padded) doubles of a table, as ctx_build.h counts them; `segments`: (n_records, n_coeffs) pairs."""
    packed = sum(n * (2 + 3 * c) for n, c in segments)
    padded = sum(n * (2 + 3 * max(c, 16)) for n, c in segments)
    return packed, padded


def almanac_sizes(al: nx.Almanac, extra=()):
    return table_sizes([(s.records.shape[0], s.n_coeffs) for s in list(al.segments) + list(extra)])


def compiled_sizes(compiled):
    cfg = compiled.cfg
    return table_sizes([(cfg.segments[i].n_records, cfg.segments[i].n_coeffs) for i in range(cfg.n_segments)])


def lds_bytes(rec_doubles: int, kind: int, reuse_fields: int = 0) -> int:
    """The library's own `nyx_kernel_lds_bytes` (a host function of libnyx_hip.so: no device is touched)."""
    lib = _abi.load_library()
    fn = lib.nyx_kernel_lds_bytes
    fn.restype, fn.argtypes = C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]
    return int(fn(16, int(rec_doubles), int(kind), int(reuse_fields)))


def fits_lds(rec_doubles: int, kind: int) -> bool:
    """`records_fit_lds` of ctx_build.h."""
    return rec_doubles <= REC_LDS_MAX and lds_bytes(rec_doubles, kind) <= KERNEL_LDS_MAX


def planned(packed: int, padded: int, build_kind: int, launch_kind: int):
    """(layout, rec_in_lds, rec_doubles) the builder and the launch should arrive at: the layout is chosen beside the context's family
    (plain, or D3 for an STM context), the placement beside the layout of the launch."""
    pad16 = not (fits_lds(packed + TAIL, build_kind) and not fits_lds(padded + TAIL, build_kind)) and padded <= PAD16_MAX
    rec = (padded if pad16 else packed) + TAIL
    return ("padded" if pad16 else "packed"), int(fits_lds(rec, launch_kind)), rec


def debug_layout(ctx):
    """`nyx_hip_debug_layout` of the last launch, as tools/time_gpu.py reads it: [waves, pipelined, carried epoch fields, chained
    attempts, records in LDS, their doubles, almanac waves, LDS bytes]."""
    lay = (C.c_int32 * 8)()
    ctx._lib.nyx_hip_debug_layout.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    assert ctx._lib.nyx_hip_debug_layout(ctx._h, lay) == 0
    return [int(v) for v in lay]


def seams(al: nx.Almanac, naif: int, lo_s: float, hi_s: float):
    """Record boundaries of the FIRST segment of a body's chain inside (lo, hi], from the segment's own init_et_s / interval_s."""
    s = al.segments[al.bodies[naif]["chain"][0][0]]
    k0 = int(np.floor((lo_s - s.init_et_s) / s.interval_s)) + 1
    k1 = int(np.floor((hi_s - s.init_et_s) / s.interval_s))
    return [s.init_et_s + k * s.interval_s for k in range(k0, k1 + 1)], s


def record_index(seg: nx.ChebySegment, et_s):
    return np.floor((np.asarray(et_s, dtype=np.float64) - seg.init_et_s) / seg.interval_s).astype(np.int64)


# lane i of `spread_batch` takes pattern i % 10:
#   0, 1      EPOCH0 itself
#   2 .. 5    40, 33, 27, 20 minutes before the next Moon / Earth (4-day) seam
#   6, 7      36, 24 minutes before the next Sun / EMB (16-day) seam, a 4-day seam as well: one run crosses both kinds
#   8         a day behind that seam
#   9         ON the 4-day seam behind it: the first evaluation of the run has t = -1 in a new record
BEFORE_SEAM_MIN = (40, 33, 27, 20)
BEFORE_BOTH_MIN = (36, 24)


def spread_epochs(n: int, al: nx.Almanac = None):
    al = al or almanac("A")
    et0 = nx.to_seconds(EPOCH0_NS)
    s4, moon = seams(al, nx.MOON, et0, et0 + 30 * DAY)
    s16, sun = seams(al, nx.SUN, et0, et0 + 30 * DAY)
    assert moon.interval_s < sun.interval_s and s4[0] < s16[0] and s16[0] in s4
    after = [s for s in s4 if s > s16[0]][0]
    for s in (s4[0], s16[0], after):
        assert float(int(s)) == s                      # whole seconds: the epochs below are exact
    S = nx.NS_PER_S
    table = ([EPOCH0_NS, EPOCH0_NS] + [int(s4[0]) * S - m * 60 * S for m in BEFORE_SEAM_MIN] +
             [int(s16[0]) * S - m * 60 * S for m in BEFORE_BOTH_MIN] + [int(s16[0]) * S + 86400 * S, int(after) * S])
    return np.array([table[i % 10] for i in range(n)], dtype=np.int64)


def spread_batch(n: int, seed: int = 0, al: nx.Almanac = None):
    """`dispersed_leo_batch(n)` with per-trajectory epochs (see the pattern above)."""
    b = dispersed_leo_batch(n, seed=seed)
    b.epoch_ns[:] = spread_epochs(n, al)
    return b


def spread_census(epoch_ns, duration_ns: int, al: nx.Almanac, lanes=slice(0, 64)):
    """What the lanes of one wave see: distinct records of the Moon's and the Sun's first segment at the start, lanes whose run
    crosses a seam of each, and how long before it they start (minutes)."""
    ep = np.asarray(epoch_ns)[lanes]
    t0 = np.array([nx.to_seconds(int(e)) for e in ep])
    t1 = np.array([nx.to_seconds(int(e) + int(duration_ns)) for e in ep])
    out = {}
    for name, naif in (("moon", nx.MOON), ("sun", nx.SUN)):
        seg = al.segments[al.bodies[naif]["chain"][0][0]]
        i0, i1 = record_index(seg, t0), record_index(seg, t1)
        nxt = seg.init_et_s + (i0 + 1) * seg.interval_s
        crossing = i1 > i0
        out[name] = dict(records=sorted(set(i0.tolist())), crossing=np.nonzero(crossing)[0], minutes_before=(nxt - t0)[crossing] / 60.0,
                         on_seam=np.nonzero(t0 == seg.init_et_s + i0 * seg.interval_s)[0])
    return out
