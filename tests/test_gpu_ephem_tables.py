"""-m gpu: the device ephemerides off every table placement and layout, and with lanes on different records.

Every other GPU test builds its context from one 40-day almanac whose sixteen-wide ("padded") records fit LDS, every lane of a wave
starting at one epoch in the middle of a record.  Here the same force models run on the four tables of tests/ephem_table_cases.py -
A padded in LDS, B packed in LDS, C padded in global memory, D packed in global memory; the leading records are the same doubles in
all four (tests/test_ephem_table_cases.py proves it on the CPU) - and on `spread_batch`, whose lanes sit on three Moon / Earth
records and two Sun / EMB records, cross the seams between them during the run, and start ON one.  After its first launch every test
reads `nyx_hip_debug_layout` and ASSERTS the placement (`rec_in_lds`) and the size (`rec_doubles` = packed + 16 or padded + 16) its
case claims: a context that lands elsewhere fails.

BOUNDS are the project's own for the same comparisons: device against the oracle after 2 h, dr < 1e-6 km and dv < 1e-9 km/s
(tests/test_abi.py, tests/test_gpu_rotation.py); Phi against the oracle under fixed steps, 1e-9 relative element-wise
(tests/test_gpu_stm_quad.py); the reports against their host definitions with the tables of tests/test_gpu_frame.py (zero for values of
+ - * / sqrt, 1e-12 deg for angles, 4e-15 relative for the period) and tests/test_gpu_eclipse.py.  Where one arithmetic runs whatever
the table (no column schedule; the reports), B, C and D must equal A BIT FOR BIT and inherit A's bound by equality."""
import os

import numpy as np
import pytest

import nyx_amd as nx
import ephem_table_cases as etc
import oracle_lib
import scenarios as sc
import test_gpu_eclipse as tge
import test_gpu_frame as tgf
from nyx_amd import _abi, ephem
from nyx_amd.eclipse import EclipseParameter as E
from nyx_amd.frames import FrameParameter as F
from rotation_cases import euler_segment_like
from test_gpu_stm_quad import stm_batch

pytestmark = pytest.mark.gpu
S = nx.NS_PER_S
DUR = 2 * 3600 * S
N = 70                       # one full wave plus six live lanes
NCPU = min(16, os.cpu_count() or 1)
TABLES = "ABCD"
DR_MAX, DV_MAX = 1e-6, 1e-9  # km, km/s: the project's bound for 2-hour runs
PHI_MAX = 1e-9               # tests/test_gpu_stm_quad.py
CENTRAL = sc.earth_frame(ephem.MU_EARTH)
# an STM context lays the records out beside the D3 layout (no table fits there: padded unless the size alone says packed); a quad
# launch then finds room for A and for B's PADDED form (3 066 doubles of the 3 072 allowed), a D3 launch for none
STM_CLAIM = {("A", 1): ("padded", 1), ("B", 1): ("padded", 1), ("C", 1): ("padded", 0), ("D", 1): ("packed", 0),
             ("A", 0): ("padded", 0), ("B", 0): ("padded", 0), ("C", 0): ("padded", 0), ("D", 0): ("packed", 0)}


def assert_layout(ctx, compiled, layout, in_lds, label):
    """The last launch of `ctx` had the records where and as wide as the case claims."""
    packed, padded = etc.compiled_sizes(compiled)
    want = (in_lds, (padded if layout == "padded" else packed) + etc.TAIL)
    lay = etc.debug_layout(ctx)
    got = (lay[4], lay[5])
    print(f"{label}: records in LDS {got[0]}, {got[1]} doubles (claimed: {layout}, in LDS {in_lds}, {want[1]} doubles)")
    assert got == want, (label, got, want)


def run(prop, name, batch, dur, stm=False, almanac=None, claim=None, label="", prepare=None):
    """One fresh context on table `name`, one launch, the layout asserted: (out, stats)."""
    compiled = prop.compile(almanac or etc.almanac(name), CENTRAL, stm=stm)
    ctx = nx.GpuContext(compiled)
    try:
        if prepare:
            prepare(ctx)
        out, st = ctx.propagate(batch, dur)
        layout, in_lds = claim or (etc.LAYOUT[name], etc.IN_LDS[name])
        assert_layout(ctx, compiled, layout, in_lds, f"{label} table {name}")
    finally:
        ctx.close()
    return out, st


def assert_same_bits(got, want, label):
    (o, s), (o0, s0) = got, want
    np.testing.assert_array_equal(s.status, s0.status, err_msg=label)
    np.testing.assert_array_equal(o.epoch_ns, o0.epoch_ns, err_msg=label)
    np.testing.assert_array_equal(s.n_evals, s0.n_evals, err_msg=label)
    np.testing.assert_array_equal(s.n_accepted, s0.n_accepted, err_msg=label)
    np.testing.assert_array_equal(o.rv(), o0.rv(), err_msg=label)


def assert_meets_oracle(out, st, ref, rst, label, ok=None):
    np.testing.assert_array_equal(st.status, rst.status, err_msg=label)
    ok = (rst.status == 0) if ok is None else ok
    np.testing.assert_array_equal(out.epoch_ns[ok], ref.epoch_ns[ok], err_msg=label)
    dr, dv = sc.pos_vel_errors(out, ref)
    print(f"{label}: worst |dr| {dr[ok].max():.3e} km, |dv| {dv[ok].max():.3e} km/s over {int(ok.sum())} runs (bounds {DR_MAX:.0e}, {DV_MAX:.0e})")
    assert dr[ok].max() < DR_MAX and dv[ok].max() < DV_MAX, (label, dr[ok].max(), dv[ok].max())


def batches():
    """The seam batch and the plain same-epoch batch."""
    return {"spread": etc.spread_batch(N, seed=21), "same-epoch": sc.dispersed_leo_batch(N, seed=21)}


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. no column schedule: one arithmetic whatever the table
# ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["spread", "same-epoch"])
def test_point_masses_and_srp_are_bit_identical_across_tables(which):
    """Sun, Moon, Jupiter + SRP with Earth and Moon shadows (`jwst_setup`'s dynamics): A meets the oracle, B, C, D equal A."""
    prop, _, _ = sc.jwst_setup()
    b = batches()[which]
    if which == "spread":
        c = etc.spread_census(b.epoch_ns, DUR, etc.almanac("A"))
        assert len(c["moon"]["records"]) >= 3 and len(c["sun"]["records"]) >= 2 and len(c["moon"]["crossing"]) >= 4 and len(c["sun"]["crossing"]) >= 2
    ref, rst = oracle_lib.propagate(prop.compile(etc.almanac("A"), CENTRAL), b, DUR, n_threads=NCPU)
    assert (rst.status == 0).all()
    got = {name: run(prop, name, b, DUR, label=f"point masses + SRP, {which},") for name in TABLES}
    assert_meets_oracle(*got["A"], ref, rst, f"point masses + SRP, {which}, A")
    for name in "BCD":
        assert_same_bits(got[name], got["A"], f"{which}: table {name} against A")


def euler_frame(et0):
    """The IAU Earth as a binary PCK holds it: two one-day records whose seam lies an hour behind EPOCH0."""
    seg = euler_segment_like(nx.IAU_EARTH_ROTATION, et0 - 23 * 3600.0, 2.0)
    return nx.Frame(nx.EARTH, ephem.MU_EARTH, sc.EARTH_RADIUS_KM, nx.Rotation(euler=seg)), seg


def test_drag_through_a_chebyshev_orientation_in_the_same_table():
    """Drag in a frame whose Euler angles are a segment of the same record table (`rotation_dcm` and its dW/dt read): the lanes start
    0, 20, 40, 60 minutes after EPOCH0, so they reach the orientation's record seam at different stages."""
    et0 = nx.to_seconds(sc.EPOCH0_NS)
    frame, seg = euler_frame(et0)
    dyn = nx.SpacecraftDynamics(nx.OrbitalDynamics([nx.PointMasses([nx.SUN, nx.MOON])]), [nx.SolarPressure.default_flux(nx.EARTH), nx.Drag.earth_exp(frame)])
    prop = nx.Propagator(dyn, nx.IntegratorMethod.RungeKutta89, nx.IntegratorOptions())
    b = sc.dispersed_leo_batch(N, seed=22)
    b.drag_area_m2[:] = 2.0
    b.epoch_ns[:] = sc.EPOCH0_NS + (np.arange(N) % 4) * 1200 * S
    t0 = np.array([nx.to_seconds(int(e)) for e in b.epoch_ns])
    i0, i1 = etc.record_index(seg, t0), etc.record_index(seg, t0 + DUR / S)
    assert (i0 >= 0).all() and (i1 < seg.records.shape[0]).all() and (i1 > i0).sum() >= N // 2 and (i1 == i0).sum() >= N // 4
    ref, rst = oracle_lib.propagate(prop.compile(etc.almanac("A"), CENTRAL), b, DUR, n_threads=NCPU)
    assert (rst.status == 0).all()
    got = {name: run(prop, name, b, DUR, label="drag, Euler / Chebyshev frame,") for name in TABLES}
    assert_meets_oracle(*got["A"], ref, rst, "drag, Euler / Chebyshev frame, A")
    for name in "BCD":
        assert_same_bits(got[name], got["A"], f"drag: table {name} against A")


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. harmonics: the launch plan may follow the placement, so every table is held to the oracle itself
# ---------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def harmonics_oracle():
    """8x8 + Sun, Moon + SRP on the seam batch: the oracle once (the four tables hold the same records: one reference)."""
    prop, _, _ = sc.leo_full_setup(degree=8)
    b = etc.spread_batch(N, seed=23)
    ref, rst = oracle_lib.propagate(prop.compile(etc.almanac("A"), CENTRAL), b, DUR, n_threads=NCPU)
    assert (rst.status == 0).all()
    return prop, b, ref, rst


@pytest.mark.parametrize("waves", [0, 16])
@pytest.mark.parametrize("name", TABLES)
def test_harmonics_meet_the_oracle_on_every_table(harmonics_oracle, name, waves):
    """`waves` = 16: the sixteen-wave pipelined kernels, whose integrator runs out of line (pk_integrator_ool.h reads the records
    through its own pointer); 0: what the planner picks."""
    prop, b, ref, rst = harmonics_oracle
    compiled = prop.compile(etc.almanac(name), CENTRAL)
    ctx = nx.GpuContext(compiled)
    try:
        if waves:
            ctx.set_column_waves(waves)
        out, st = ctx.propagate(b, DUR)
        label = f"8x8, {waves or 'planned'} waves, table {name}"
        assert_layout(ctx, compiled, etc.LAYOUT[name], etc.IN_LDS[name], label)
        lay = etc.debug_layout(ctx)
        print(f"{label}: waves {lay[0]}, pipelined {lay[1]}")
        if waves:
            assert lay[0] == 16 and lay[1] == 1
    finally:
        ctx.close()
    assert_meets_oracle(out, st, ref, rst, label)


@pytest.fixture(scope="module")
def stm_oracle():
    prop, _, _ = sc.leo_full_setup(degree=8, opts=nx.IntegratorOptions.with_fixed_step_s(30.0))
    b = stm_batch(N, seed=24, geo_tail=False)
    b.epoch_ns[:] = etc.spread_epochs(N)
    ref, rst = oracle_lib.propagate(prop.compile(etc.almanac("A"), CENTRAL, stm=True), b, DUR, n_threads=NCPU)
    assert (rst.status == 0).all()
    return prop, b, ref, rst


@pytest.mark.parametrize("quad", [1, 0])
@pytest.mark.parametrize("name", TABLES)
def test_stm_meets_the_oracle_on_every_table_and_layout(stm_oracle, name, quad):
    """Fixed 30 s steps: the oracle's step sequence; states at the 2-hour bound, Phi at the bound of tests/test_gpu_stm_quad.py."""
    prop, b, ref, rst = stm_oracle
    label = f"STM 8x8, {'quad' if quad else 'D3'} layout,"
    out, st = run(prop, name, b, DUR, stm=True, claim=STM_CLAIM[(name, quad)], label=label, prepare=lambda ctx: ctx.set_stm_layout(quad))
    assert_meets_oracle(out, st, ref, rst, f"{label} table {name}")
    a, r = out.stm.reshape(-1, 81), ref.stm.reshape(-1, 81)
    scale = np.maximum(np.abs(r), 1e-6 * np.abs(r).max(axis=1, keepdims=True))
    err = (np.abs(a - r) / scale).max()
    print(f"{label} table {name}: worst Phi element {err:.3e} relative (bound {PHI_MAX:.0e})")
    assert err < PHI_MAX


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. wide segments from global memory
# ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ncoef", [16, 32])
def test_wide_coefficient_segments_from_global_memory(ncoef):
    """`test_wide_coefficient_segments_device_vs_oracle` (tests/test_abi.py) with the Moon's segment continued by never-visited
    records until the table leaves LDS: the sixteen-wide window (16) and the rolled loop (32) on global loads."""
    day = 86400.0
    et0 = nx.to_seconds(sc.EPOCH0_NS)

    def almanac_with(last):
        al = nx.Almanac()
        s_sun = al.add_segment(ephem.fit_segment(ephem.sun_geocentric, et0 - 2 * day, 16 * day, 2, 16))
        moon = ephem.fit_segment(ephem.moon_geocentric, et0 - 2 * day, 8 * day, 3, ncoef)
        for c in range(3):
            moon.records[:, 2 + ncoef * c + ncoef - 1] = last    # a LARGE last coefficient (synthetic table): dropping it moves the Moon by up to 500 km
        s_moon = al.add_segment(etc.extend_segment(moon, 60))
        al.add_body(nx.EARTH, ephem.MU_EARTH, ephem.R_EARTH, [])
        al.add_body(nx.SUN, ephem.MU_SUN, ephem.R_SUN, [(s_sun, +1)])
        al.add_body(nx.MOON, ephem.MU_MOON, ephem.R_MOON, [(s_moon, +1)])
        return al

    al = almanac_with(500.0)
    prop, _, _ = sc.leo_full_setup(degree=4)
    b = sc.dispersed_leo_batch(N, seed=16)
    packed, padded = etc.almanac_sizes(al)
    assert packed == padded and not etc.fits_lds(packed + etc.TAIL, etc.PLAIN)
    out, st = run(prop, "wide", b, DUR, almanac=al, claim=("packed", 0), label=f"{ncoef} coefficients,")
    ref, rst = oracle_lib.propagate(prop.compile(al, CENTRAL), b, DUR, n_threads=NCPU)
    assert (rst.status == 0).all()
    assert_meets_oracle(out, st, ref, rst, f"{ncoef} coefficients from global memory")
    # ... and the coefficient matters at the level of this comparison: without it the oracle itself lands > 1 mm elsewhere
    ref0, _ = oracle_lib.propagate(prop.compile(almanac_with(0.0), CENTRAL), b, DUR, n_threads=NCPU)
    moved = sc.pos_vel_errors(ref0, ref)[0].max()
    print(f"{ncoef} coefficients: the last one moves the oracle by {moved:.3e} km")
    assert moved > 1e-6


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. a stage epoch ON a seam, a final epoch ON the end of the table
# ---------------------------------------------------------------------------------------------------------------------------------

STEP_FIXED = 60 * S


def seam_and_end_epochs(al, overshoot_ns):
    """Lane i takes pattern i % 7 (fixed 60 s steps, 120 of them; every seam and the end are whole seconds):
        0  EPOCH0: the middle of the table
        1  30 steps before a Moon / Earth seam: a step starts ON it (t = -1 in the new record) and the step before ends ON it
        2  45 steps before the Sun / EMB seam
        3  starts ON a Moon / Earth seam
        4  its LAST stage epoch in time IS the earliest end of the table (idx == n_rec and et == end_et: allowed)
        5  one step later: its last step leaves the table - ERR_EPHEM_RANGE
        6  one step earlier: ends a step short of it
    `overshoot_ns`: how far the method's stages reach beyond the end of a step (RK89: c_11 = 4 / 3, 20 s of a 60 s step; Dormand-Prince
    4(5): nothing - there the run's FINAL EPOCH is the end of the table)."""
    et0 = nx.to_seconds(sc.EPOCH0_NS)
    s4, _ = etc.seams(al, nx.MOON, et0, et0 + 30 * etc.DAY)
    s16, _ = etc.seams(al, nx.SUN, et0, et0 + 30 * etc.DAY)
    end_s = min(s.init_et_s + s.interval_s * s.records.shape[0] for s in al.segments)
    for v in (s4[0], s4[1], s16[0], end_s):
        assert float(int(v)) == v
    last = int(end_s) * S - overshoot_ns - DUR
    table = [sc.EPOCH0_NS, int(s4[0]) * S - 30 * STEP_FIXED, int(s16[0]) * S - 45 * STEP_FIXED, int(s4[1]) * S, last, last + STEP_FIXED, last - STEP_FIXED]
    return np.array([table[i % 7] for i in range(N)], dtype=np.int64), int(end_s) * S


@pytest.mark.parametrize("method,overshoot_s", [(nx.IntegratorMethod.RungeKutta89, 20), (nx.IntegratorMethod.DormandPrince45, 0)])
@pytest.mark.parametrize("name", "ABC")     # (D ends ninety years on, beyond the century the device's epoch arithmetic states)
def test_a_stage_epoch_on_a_seam_and_on_the_end_of_the_table(name, method, overshoot_s):
    al = etc.almanac(name)
    prop, _, _ = sc.jwst_setup(opts=nx.IntegratorOptions.with_fixed_step(STEP_FIXED), method=method)
    b = sc.dispersed_leo_batch(N, seed=25)
    b.epoch_ns[:], end_ns = seam_and_end_epochs(al, overshoot_s * S)
    assert DUR % STEP_FIXED == 0
    compiled = prop.compile(al, CENTRAL)
    ref, rst = oracle_lib.propagate(compiled, b, DUR, n_threads=NCPU)
    pattern = np.arange(N) % 7
    np.testing.assert_array_equal(rst.status, np.where(pattern == 5, _abi.ERR_EPHEM_RANGE, 0))      # the oracle: only the late lane leaves the table
    assert (ref.epoch_ns[pattern == 4] == end_ns - overshoot_s * S).all()
    label = f"{method.name}, on the seam / on the end,"
    out, st = run(prop, name, b, DUR, label=label)
    assert_meets_oracle(out, st, ref, rst, f"{label} table {name}")


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. the reports on seams and on the packed layout
# ---------------------------------------------------------------------------------------------------------------------------------

REPORT_STEP = 60 * S
REPORT_COUNT = 121
SUN_PARAMS = [F.X, F.VZ, F.Rmag, F.Eccentricity, F.C3, F.BdotT, F.BdotR, F.VInfinity]


@pytest.fixture(scope="module")
def reports():
    """`spread_batch` through 8x8 with dense output on table A, its `traj_every` states and the host definitions on them: once."""
    al = etc.almanac("A")
    prop, _, _ = sc.leo_full_setup(degree=8)
    compiled = prop.compile(al, CENTRAL)
    ctx = nx.GpuContext(compiled)
    try:
        _, st, traj = ctx.propagate_with_traj(etc.spread_batch(N, seed=11), DUR, capacity=256)
        assert_layout(ctx, compiled, "padded", 1, "reports: the run, table A")
        assert (st.status == 0).all()
        ev = ctx.traj_every(traj, REPORT_STEP, REPORT_COUNT)
    finally:
        ctx.close()
    assert (ev.len == REPORT_COUNT).all()
    rv = np.ascontiguousarray(ev.state.transpose(1, 2, 0))             # [K, n, 6]
    world = dict(almanac=al, central=CENTRAL, model=nx.ShadowModel.cislunar(al), moon=al.frame_info(nx.MOON), sun=al.frame_info(nx.SUN))
    # the samples straddle record seams: of at least four trajectories, and inside one tile of eight samples
    seg = al.segments[al.bodies[nx.MOON]["chain"][0][0]]
    t = np.array([[nx.to_seconds(int(e)) for e in row] for row in ev.epoch_ns[:REPORT_COUNT]])      # [K, n]
    idx = etc.record_index(seg, t)
    straddling = np.nonzero(idx.min(axis=0) != idx.max(axis=0))[0]
    tiles = idx[: REPORT_COUNT // 8 * 8].reshape(-1, 8, N)            # FRM_TILE of csrc/frame_kernel.hip (the eclipse kernel's sixteen: two of these)
    split_tiles = int((tiles.min(axis=1) != tiles.max(axis=1)).sum())
    on_seam = int((t == seg.init_et_s + idx * seg.interval_s).sum())
    print(f"reports: {len(straddling)} trajectories straddle a Moon / Earth seam, {split_tiles} tiles of eight hold both sides, {on_seam} samples ON a seam")
    assert len(straddling) >= 4 and split_tiles >= 1 and on_seam >= 1
    want = dict(moon=tgf.host_values(world, tgf.ALL, rv, ev.epoch_ns, world["moon"]), sun=tgf.host_values(world, SUN_PARAMS, rv, ev.epoch_ns, world["sun"]),
                ecl=tge.host_values(world, tge.ALL, rv, ev.epoch_ns), ecl_moon=tge.host_values(world, tge.MOON, rv, ev.epoch_ns))
    tge.assert_no_decision_can_flip(world, rv, ev.epoch_ns)
    return world, prop, traj, want


def device_reports(ctx, world, traj):
    out = {}
    out["moon"], l1 = ctx.traj_frame_values(traj, world["moon"], tgf.ALL, REPORT_STEP, capacity=REPORT_COUNT)
    out["sun"], l2 = ctx.traj_frame_values(traj, world["sun"], SUN_PARAMS, REPORT_STEP, capacity=REPORT_COUNT)
    out["ecl"], l3 = ctx.traj_eclipse(traj, world["model"], tge.ALL, REPORT_STEP, capacity=REPORT_COUNT)
    out["ecl_moon"], l4 = ctx.traj_eclipse(traj, world["model"], tge.MOON, REPORT_STEP, capacity=REPORT_COUNT)
    for l in (l1, l2, l3, l4):
        assert (l == REPORT_COUNT).all()
    return out


def test_reports_on_seams_and_on_the_packed_layout(reports):
    world, prop, traj, want = reports
    got = {}
    for name in TABLES:
        compiled = prop.compile(etc.almanac(name), CENTRAL)
        ctx = nx.GpuContext(compiled)
        try:
            ctx.propagate(sc.dispersed_leo_batch(2, seed=1), 60 * S)                  # a launch: the layout of this context
            assert_layout(ctx, compiled, etc.LAYOUT[name], etc.IN_LDS[name], f"reports, table {name}")
            got[name] = device_reports(ctx, world, traj)
        finally:
            ctx.close()
    tgf.assert_all_within(tgf.ALL, got["A"]["moon"], want["moon"], label=" seams, moon")
    tgf.assert_all_within(SUN_PARAMS, got["A"]["sun"], want["sun"], label=" seams, sun")
    tge.assert_all_within(tge.ALL, got["A"]["ecl"], want["ecl"], label=" seams")
    tge.assert_all_within(tge.MOON, got["A"]["ecl_moon"], want["ecl_moon"], label=" seams, moon")
    for name in "BCD":
        for key in ("moon", "sun", "ecl", "ecl_moon"):
            np.testing.assert_array_equal(got[name][key], got["A"][key], err_msg=f"table {name}, {key}")
    print("reports: tables B, C, D equal A bit for bit (frame values about the Moon and the Sun, eclipses of the Earth and the Moon)")


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. rec_in_lds flipping inside one context
# ---------------------------------------------------------------------------------------------------------------------------------

def test_records_move_between_lds_and_global_memory_inside_one_context():
    """Table A (2 366 doubles) fits beside the quad STM layout (room for 3 136) and not beside the D3 one (1 216): quad, D3, quad on
    ONE context flips `rec_in_lds` twice, and every launch equals a fresh context's bit for bit."""
    packed, padded = etc.almanac_sizes(etc.almanac("A"))
    assert etc.fits_lds(padded + etc.TAIL, etc.QUAD) and not etc.fits_lds(padded + etc.TAIL, etc.D3) and not etc.fits_lds(packed + etc.TAIL, etc.D3)
    prop, _, _ = sc.leo_full_setup(degree=8)
    compiled = prop.compile(etc.almanac("A"), CENTRAL, stm=True)
    b = stm_batch(N, seed=26, geo_tail=False)
    b.epoch_ns[:] = etc.spread_epochs(N)
    dur = 1800 * S

    def fresh(quad):
        ctx = nx.GpuContext(compiled)
        try:
            ctx.set_stm_layout(quad)
            ctx.set_column_waves(4)
            return ctx.propagate(b, dur)
        finally:
            ctx.close()

    want = {1: fresh(1), 0: fresh(0)}
    ctx = nx.GpuContext(compiled)
    try:
        ctx.set_column_waves(4)
        for k, quad in enumerate((1, 0, 1)):
            ctx.set_stm_layout(quad)
            out, st = ctx.propagate(b, dur)
            assert_layout(ctx, compiled, "padded", quad, f"launch {k} ({'quad' if quad else 'D3'}) of one context")
            assert (st.status == 0).all()
            assert_same_bits((out, st), want[quad], f"launch {k}")
            np.testing.assert_array_equal(out.stm, want[quad][0].stm)
    finally:
        ctx.close()
    # (same column split: the two layouts agree with each other too, tests/test_gpu_stm_quad.py)
    np.testing.assert_array_equal(want[1][0].stm, want[0][0].stm)
