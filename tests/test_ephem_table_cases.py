"""CPU: the four almanacs of tests/ephem_table_cases.py share their leading records bit for bit, fall on the intended sides of the
sizes nyx_amd/csrc/ctx_build.h decides by, and compile to configurations nyx_hip_ctx_create accepts; `spread_batch` puts the lanes of
one wave on different records and across record seams.  What tests/test_gpu_ephem_tables.py relies on, proved without a GPU."""
import ctypes as C
import time

import numpy as np
import pytest

import nyx_amd as nx
import ephem_table_cases as etc
from nyx_amd import _abi
from scenarios import EPOCH0_NS, jwst_setup

S = nx.NS_PER_S
D_BUILD_BUDGET_S = 5.0     # "a few seconds"; the copies take milliseconds beyond C's fits


def test_leading_records_are_bit_identical():
    a = etc.almanac("A")
    assert len(a.segments) == 5
    for name in "BCD":
        other = etc.almanac(name)
        assert len(other.segments) == len(a.segments) and other.bodies == a.bodies
        for sa, so in zip(a.segments, other.segments):
            n = sa.records.shape[0]
            assert so.init_et_s == sa.init_et_s and so.interval_s == sa.interval_s and so.records.shape[1] == sa.records.shape[1]
            assert so.records.shape[0] >= n
            assert so.records[:n].tobytes() == sa.records.tobytes()           # the same doubles, not merely equal values
        assert sum(s.records.shape[0] for s in other.segments) > sum(s.records.shape[0] for s in a.segments)
    # D beyond C: the midpoints go on, record by record, to the end build_almanac would give that span
    c, d = etc.almanac("C"), etc.almanac("D")
    for sc_, sd in zip(c.segments, d.segments):
        n = sc_.records.shape[0]
        assert sd.records[:n].tobytes() == sc_.records.tobytes()
        mids = sd.init_et_s + (np.arange(sd.records.shape[0]) + 0.5) * sd.interval_s
        np.testing.assert_array_equal(sd.records[:, 0], mids)
        assert (sd.records[:, 1] == sd.interval_s / 2.0).all()
        assert sd.init_et_s + sd.interval_s * sd.records.shape[0] >= nx.to_seconds(EPOCH0_NS) + etc.SPAN_DAYS["D"] * etc.DAY


def test_the_library_carve_leaves_the_room_the_cases_are_sized_for():
    """`nyx_kernel_lds_bytes` itself (a host function of the library): the largest table beside each layout."""
    room = {k: max(r for r in range(0, 4000, 2) if etc.lds_bytes(r, k) <= etc.KERNEL_LDS_MAX) for k in (etc.PLAIN, etc.D3, etc.QUAD)}
    print("records beside the plain / D3 / quad layout:", room)
    assert room == {etc.PLAIN: 2560, etc.D3: 1216, etc.QUAD: 3136}
    assert etc.lds_bytes(100, etc.PLAIN) - etc.lds_bytes(0, etc.PLAIN) == 800


def test_sizes_fall_on_the_intended_sides():
    sizes = {n: etc.almanac_sizes(etc.almanac(n)) for n in "ABCD"}
    print(sizes)
    assert sizes["A"] == (1852, 2350)
    for name, (packed, padded) in sizes.items():
        layout, in_lds, rec = etc.planned(packed, padded, etc.PLAIN, etc.PLAIN)
        assert (layout, in_lds) == (etc.LAYOUT[name], etc.IN_LDS[name]), (name, layout, in_lds)
        assert rec == (padded if layout == "padded" else packed) + etc.TAIL
    pa, pd_ = sizes["A"]
    assert etc.fits_lds(pd_ + 16, etc.PLAIN)                                                     # A: even the padded table fits
    pb, pdb = sizes["B"]
    assert etc.fits_lds(pb + 16, etc.PLAIN) and not etc.fits_lds(pdb + 16, etc.PLAIN) and pb + 16 <= 3072
    pc, pdc = sizes["C"]
    assert pc > 3072 and pdc <= 2 ** 20
    pdd = sizes["D"][1]
    assert pdd > 2 ** 20 and sum(s.records.shape[0] for s in etc.almanac("D").segments) > 21000
    # an STM context decides beside the D3 layout, where none of the four fits: A - C stay padded, D is packed by its size alone;
    # a quad launch then finds A and B in LDS, a D3 launch finds nothing there
    for name, (packed, padded) in sizes.items():
        layout, lds_q, rec = etc.planned(packed, padded, etc.D3, etc.QUAD)
        assert layout == ("packed" if name == "D" else "padded") and lds_q == (1 if name in "AB" else 0)
        assert etc.planned(packed, padded, etc.D3, etc.D3)[1] == 0


@pytest.mark.parametrize("name", "ABCD")
def test_the_compiled_configuration_passes_ctx_create(name):
    prop, _, central = jwst_setup()
    cc = prop.compile(etc.almanac(name), central)
    assert etc.compiled_sizes(cc) == etc.almanac_sizes(etc.almanac(name))
    lib = _abi.load_library()
    h = C.c_void_p()
    rc = lib.nyx_hip_ctx_create(C.byref(cc.cfg), 0, C.byref(h))
    if rc == 0:
        lib.nyx_hip_ctx_destroy(h)
    assert rc in (0, _abi.RC_NO_DEVICE), _abi.last_error()


def test_table_d_builds_inside_its_budget():
    from nyx_amd import ephem
    t0 = time.perf_counter()          # from nothing: C's fits, then the copies
    c = ephem.build_almanac(nx.to_seconds(EPOCH0_NS), etc.SPAN_DAYS["C"])
    d = etc.extended(c, nx.to_seconds(EPOCH0_NS), etc.SPAN_DAYS["D"])
    dt = time.perf_counter() - t0
    assert all(x.records.tobytes() == y.records.tobytes() for x, y in zip(d.segments, etc.almanac("D").segments))
    print(f"table D: {sum(s.records.shape[0] for s in d.segments)} records, {etc.almanac_sizes(d)} doubles, built in {dt:.3f} s")
    assert dt < D_BUILD_BUDGET_S


def test_spread_batch_puts_one_wave_on_different_records_and_across_seams():
    a = etc.almanac("A")
    dur = 2 * 3600 * S
    b = etc.spread_batch(70, seed=21)
    assert b.n == 70 and (b.epoch_ns >= EPOCH0_NS).all()
    for lanes in (slice(0, 64), slice(0, 70)):
        c = etc.spread_census(b.epoch_ns, dur, a, lanes)
        assert len(c["moon"]["records"]) >= 3 and len(c["sun"]["records"]) >= 2
        m = c["moon"]["minutes_before"]
        assert ((m >= 20.0) & (m <= 40.0)).sum() >= 4 and len(c["moon"]["crossing"]) >= 4
        s = c["sun"]["minutes_before"]
        assert ((s >= 20.0) & (s <= 40.0)).sum() >= 2
        assert set(c["sun"]["crossing"]) <= set(c["moon"]["crossing"])          # one run crosses both kinds
        assert len(c["moon"]["on_seam"]) >= 1 and not len(c["sun"]["on_seam"])
    # the last wave (6 live lanes) has seam lanes of its own
    tail = etc.spread_census(b.epoch_ns, dur, a, slice(64, 70))
    assert len(tail["moon"]["crossing"]) >= 2 and len(tail["sun"]["crossing"]) >= 1 and len(tail["moon"]["records"]) >= 3
    # every record a run visits is one of A's - the shortest table - hence of all four
    for s_ in a.segments:
        i1 = etc.record_index(s_, [nx.to_seconds(int(e) + dur) for e in b.epoch_ns])
        assert (i1 < s_.records.shape[0]).all() and (etc.record_index(s_, [nx.to_seconds(int(e)) for e in b.epoch_ns]) >= 0).all()
    # the states are dispersed_leo_batch's
    from scenarios import dispersed_leo_batch
    np.testing.assert_array_equal(b.rv(), dispersed_leo_batch(70, seed=21).rv())
