"""Lambert transfers on the MI355X (lambert_kernel.hip, include/nyx_hip_lambert.h) against the host definition nyx_amd/lambert.py.

Small on purpose: batches of 70 problems (one full wave plus six live lanes), 1 and 0; grids of a few hundred cells on the 40-day
almanac of `leo_full_setup(degree=0)`.  The definition is evaluated once per case on the CPU and shared.

WHAT IS COMPARED.  `status` and Iterations exactly, everywhere.  The values under the bounds below in every cell whose
`decision_margin` (the smallest relative distance of a branch-deciding comparison of the definition - the stop tests, T against T_0 and
T_1, the series window, the m_max refinement, dnu against pi - from equality) is at least 1e-6; the fixtures assert on the CPU that this
holds for EVERY cell of every case here (up to 1 % of a case could be left out of the value comparison; none is).

BOUNDS, from the number formats and the documented accuracy of the functions, not from a run.  eps = 2^-52.
The solver's arithmetic is + - * / sqrt in one order on both sides (csrc/lambert_dev.h restates the definition operation for operation,
-ffp-contract=off): given equal inputs it is bit for bit.  What differs is libm: on the path of the LAST Householder step (the method's
order wipes out what the step inherited: a difference d of its starting point comes out as O(step^3) d, below 1e-12 d at tol = 1e-4)
stands one inverse function, psi = atan2(sin psi, cos psi) or asinh(..) - the device's within 6 and 4 ulp (the OpenCL bounds ROCm's
device library documents), glibc's within 1 and 2: at most 7 ulp of psi, hence of T (psi enters T with a factor of at most 1 relative to
T's own terms: the definition forms y - lam x and x - lam y without cancellation, see its departure 4) - and then
twelve roundings between psi and the new x ((psi + m pi) / sqrt|den|, - x, + lam y, / den, - T, the three derivatives, num, den, num /
den, fval *, p0 -) that may fall differently once psi differs, an ulp each at most: 7 + 12 = 19.  K = 18 is held, the sum first derived when psi was an
acos (4 + 2 ulp): the tighter of the two.  An error dT of T moves the root by
dT / T', so
    |dx| <= K eps (|T / T'| + |x|)
    |dv| <= K eps (|T / T'| |dv/dx| + |v|)          for the vectors v_init and v_final, in the Euclidean norm
with T' and dv/dx per cell from the host definition (`extras` of lambert.solve).  On the series path (x > 0 next to 1) no libm call is
made and the same bound holds with room.
TofS: zero (integer nanoseconds to seconds, the project's rule, on both sides; the batch copies its input).
TransferAngleDeg: acos of bit-identical input, 4 + 1 ulp of at most pi rad, scaled: the siblings' 1e-12 deg.
C3 = |w|^2, w = v_init - v_body1: 2 |w| |dv| + 4 eps C3.  VinfDep: |dv| + 2 eps |w|.  VinfArr: the same with v_final.  DvTotal: their sum
plus eps of the value.  RlaDeg = atan2(w.y, w.x): the direction moves by at most |dv| / |w_xy| rad, plus atan2's 6 + 1 ulp: 1e-12 deg.
DlaDeg = asin(w.z / |w|): the declination moves by at most the angle between w and w', |dv| / |w| rad, plus the rounding of the ratio
and asin's 4 + 1 ulp through asin' = 1 / cos(dla): 8 eps / cos(dla) rad, plus 1e-12 deg.

MEASURED on the MI355X (printed per parameter by every test; profiles/HISTORY.md): over all 22 cases the largest deviation is 0.19 of
its bound (X, a batch), the velocities 0.14, the angles 0.06.

The Earth -> Moon grid about the Sun (test_4) is what the definition's departure 4 was found on: r1 and r2 are 0.003 .. 0.07 of their
length apart, lam = 0.97, psi = 0.025.  With psi = acos(x y + lam (1 - x x)) and T's numerator as (psi / sqrt - x) + lam y, as the
reference writes them, half an ulp of the acos argument is 1.1e-16 / sin(psi) in psi, and a one-ulp difference of the last step's
starting point re-rolls that rounding: X deviated by 1.5e-13, 25 times this bound (the velocities 22 times), and the host definition
moved its own root by 53 times the bound when its start was moved by 2 ulp.  With psi from its sine and cosine the case sat at 1.25
times the bound (the cancellation of x - lam y, 0.0004 out of 0.7, in a T of 0.07); with both differences factored, at 0.09.  The bound
and K were the same throughout."""
import ctypes as C

import numpy as np
import pytest

import nyx_amd as nx
from nyx_amd import _abi, lambert
from nyx_amd.lambert import LambertParameter as P, LambertStatus as St, TransferKind as Way
from lambert_cases import MARGIN, MU_EARTH, bounds, problems
from scenarios import EPOCH0_NS, leo_full_setup

pytestmark = pytest.mark.gpu

S = nx.NS_PER_S
DAY = 86400 * S
ALL = list(P)          # sixteen: two launches through the Python split


def compare(label, grid, want, status, extras, rv1, rv2):
    """`grid` (a LambertGrid of ALL) against the definition, flattened to [16, N]: status and Iterations exactly, NaN exactly where the
    status is not OK, every value within its bound; prints the largest deviation per parameter in units of its bound."""
    got = np.stack([grid.of(p) for p in ALL]).reshape(len(ALL), -1)
    want, status = want.reshape(len(P), -1), status.reshape(-1)
    margin = np.array([ex["decision_margin"] for ex in extras])
    solved = status == St.OK
    assert (margin[solved] >= MARGIN).all(), f"{label}: decision_margin {margin[solved].min():.2e} in a compared cell: choose other inputs"
    np.testing.assert_array_equal(grid.status.reshape(-1), status, err_msg=f"{label}: status")
    np.testing.assert_array_equal(np.isnan(got), np.broadcast_to(~solved, got.shape), err_msg=f"{label}: NaN pattern")
    np.testing.assert_array_equal(got[P.Iterations][solved], want[P.Iterations][solved], err_msg=f"{label}: Iterations")
    bound = bounds(want, extras, rv1, rv2)
    failures = []
    for p in ALL:
        d = np.abs(got[p][solved] - want[p][solved])
        if p in (P.RlaDeg,):
            d = np.abs((got[p][solved] - want[p][solved] + 180.0) % 360.0 - 180.0)
        b = bound[p][solved]
        worst = float(d.max()) if d.size else 0.0
        ratio = float(np.max(np.where(b > 0.0, d / np.where(b > 0.0, b, 1.0), np.where(d > 0.0, np.inf, 0.0)))) if d.size else 0.0
        print(f"deviation {label} {p.name:16s} {worst:.3e}  ({ratio:.3f} of its bound, {int(solved.sum())} values)")
        if not (d <= b).all():
            failures.append(f"{label} {p.name}: {worst:.3e}, {ratio:.2f} of its bound")
    assert not failures, "\n".join(failures)


@pytest.fixture(scope="module")
def world():
    prop, almanac, central = leo_full_setup(degree=0)
    ctx = nx.GpuContext(prop.compile(almanac, central))
    frames = {k: almanac.frame_info(b) for k, b in (("sun", nx.SUN), ("moon", nx.MOON), ("jupiter", nx.JUPITER_BARYCENTER), ("earth", central.naif_id))}
    yield dict(prop=prop, almanac=almanac, central=central, ctx=ctx, **frames)
    ctx.close()


BATCH = problems()
assert (np.cross(BATCH[0][:3, :60].T, BATCH[1][:3, :60].T)[:, 2] < 0.0).sum() == 30


@pytest.mark.parametrize("way", list(Way))
@pytest.mark.parametrize("n_revs,high_path", [(0, 0), (1, 0), (1, 1), (2, 0), (2, 1)])
def test_1_batch_of_70_every_way_revolution_and_path(world, way, n_revs, high_path):
    rv1, rv2, tof = BATCH
    want, status, extras = lambert.batch_definition(rv1, rv2, tof, MU_EARTH, way, n_revs, high_path)
    seen = set(status.tolist())
    assert {St.OK, St.BAD_INPUT, St.DEGENERATE} <= seen and (St.NOT_FEASIBLE if n_revs else St.TOO_CLOSE) in seen   # (too short for a revolution)
    got = world["ctx"].lambert_batch(rv1, rv2, tof, MU_EARTH, ALL, way, n_revs, high_path)
    assert got.values.shape == (16, 70) and got.status.dtype == np.int32
    compare(f"batch {way.name} m={n_revs} hp={high_path}", got, want, status, extras, rv1, rv2)
    if n_revs == 0 and way is not Way.Auto:   # Vallado 7-1, the reference's own unit test, from the device
        v = got.values[:6, 69]
        exp = {Way.ShortWay: [2.058913, 2.915965, 0.0, -3.451565, 0.910315, 0.0], Way.LongWay: [-3.811158, -2.003854, 0.0, 4.207569, 0.914724, 0.0]}[way]
        assert np.linalg.norm(v[:3] - exp[:3]) < 1e-5 and np.linalg.norm(v[3:] - exp[3:]) < 1e-5


def test_2_iteration_limit_one_problem_and_none(world):
    ctx = world["ctx"]
    rv1, rv2, tof = BATCH
    want, status, extras = lambert.batch_definition(rv1, rv2, tof, MU_EARTH, Way.Auto, tol=1e-10, max_iter=2)
    assert {St.OK, St.MAX_ITER} <= set(status.tolist())
    compare("batch max_iter=2", ctx.lambert_batch(rv1, rv2, tof, MU_EARTH, ALL, Way.Auto, tol=1e-10, max_iter=2), want, status, extras, rv1, rv2)
    one = ctx.lambert_batch(rv1[:, 3:4], rv2[:, 3:4], tof[3:4], MU_EARTH, ALL, Way.ShortWay)
    w1, s1, e1 = lambert.batch_definition(rv1[:, 3:4], rv2[:, 3:4], tof[3:4], MU_EARTH, Way.ShortWay)
    compare("batch n=1", one, w1, s1, e1, rv1[:, 3:4], rv2[:, 3:4])
    none = ctx.lambert_batch(np.zeros((6, 0)), np.zeros((6, 0)), np.zeros(0), MU_EARTH, [P.C3])
    assert none.values.shape == (1, 0) and none.status.shape == (0,) and none.best(P.C3) is None and none.feasible_fraction == 0.0
    with pytest.raises(ValueError, match="tol"):
        ctx.lambert_batch(rv1, rv2, tof, MU_EARTH, [P.C3], tol=1e-1)
    with pytest.raises(TypeError):
        ctx.lambert_batch(rv1, rv2, tof, MU_EARTH, [nx.FrameParameter.C3])


def run_grid(world, label, dep, arr, centre, n_dep, n_arr, **kw):
    """The device's grid of ALL against the definition; returns (LambertGrid, want, status)."""
    want, status, extras, dep_ns, arr_ns = lambert.grid_definition(world[dep], world[arr], world[centre], world["almanac"], world["central"], n_dep, n_arr, **kw)
    solver = {"kind": kw.pop("way")} if "way" in kw else {}
    got = world["ctx"].lambert_grid(world[dep], world[arr], world[centre], ALL, n_dep, n_arr, **kw, **solver)
    assert got.values.shape == (16, n_dep, n_arr) and got.status.shape == (n_dep, n_arr)
    np.testing.assert_array_equal(got.dep_ns, dep_ns)
    np.testing.assert_array_equal(got.arr_ns, arr_ns)
    rv1, rv2, _ = lambert.grid_states(world[dep], world[arr], world[centre], dep_ns, arr_ns, world["almanac"], world["central"])
    rv1 = np.broadcast_to(rv1[:, None, :], rv2.shape).reshape(-1, 6).T
    compare(label, got, want, status, [e for row in extras for e in row], rv1, rv2.reshape(-1, 6).T)
    return got, want, status


def test_3_earth_to_jupiter_about_the_sun_with_statistics(world):
    """5 x 70, hyperbolic (x > 1, the asinh branch), arrivals by epoch: a partial tile in both directions."""
    got, want, status = run_grid(world, "earth-jupiter", "earth", "jupiter", "sun", 5, 70, dep0_ns=EPOCH0_NS + DAY // 2, dep_step_ns=DAY,
                                 arr0_ns=EPOCH0_NS + 10 * DAY, arr_step_ns=2 * DAY // 5)
    assert (status == St.OK).all() and (want[P.X] > 1.0).all() and got.feasible_fraction == 1.0
    c3 = got.of(P.C3)
    value, (i, j), dep_ns, arr_ns = got.best(P.C3)
    assert value == c3.min() and c3[i, j] == value and dep_ns == got.dep_ns[i] and arr_ns == got.arr_ns[i, j]
    # the values block is a [rows, capacity, n] block of the statistics: minimum C3 of every departure and its arrival
    stats = world["ctx"].series_stats(got.values[[ALL.index(P.C3)]], np.full(70, 5, dtype=np.int32))
    np.testing.assert_array_equal(stats[0, :, nx.Stat.MIN], c3.min(axis=1))
    np.testing.assert_array_equal(stats[0, :, nx.Stat.ARGMIN], c3.argmin(axis=1))


def test_4_earth_to_moon_by_time_of_flight_about_the_sun(world):
    """70 x 3: nine departure tiles, the last with six live rows; three live lanes; every lane evaluates its own arrival state."""
    _, _, status = run_grid(world, "earth-moon tof", "earth", "moon", "sun", 70, 3, dep0_ns=EPOCH0_NS + DAY // 4, dep_step_ns=DAY // 4, tof0_ns=3 * DAY,
                            tof_step_ns=5 * DAY)
    assert (status == St.OK).all()


@pytest.mark.parametrize("n_revs", [0, 1])
def test_5_moon_to_moon_about_the_earth(world, n_revs):
    """3 departures x 40 days in 1-day steps: across the 180 deg transfer and the near-closed chord at one lunar period; with one
    revolution nothing is feasible before about one period."""
    _, want, status = run_grid(world, f"moon-moon m={n_revs}", "moon", "moon", "earth", 3, 40, dep0_ns=EPOCH0_NS + DAY // 8, dep_step_ns=DAY // 4, tof0_ns=DAY,
                               tof_step_ns=DAY, n_revs=n_revs)
    if n_revs:
        assert (status[:, :20] == St.NOT_FEASIBLE).all() and (status[:, 30:] == St.OK).all()
    else:
        assert (status == St.OK).all() and want[P.TransferAngleDeg].min() < 30.0 and want[P.TransferAngleDeg].max() > 330.0


def test_6_one_cell_arrivals_before_departures_and_the_end_of_the_table(world):
    run_grid(world, "1 x 1", "earth", "moon", "sun", 1, 1, dep0_ns=EPOCH0_NS, dep_step_ns=DAY, arr0_ns=EPOCH0_NS + 4 * DAY, arr_step_ns=DAY, way=Way.LongWay)
    _, _, status = run_grid(world, "arrivals first", "earth", "moon", "sun", 4, 6, dep0_ns=EPOCH0_NS + 2 * DAY, dep_step_ns=DAY, arr0_ns=EPOCH0_NS, arr_step_ns=DAY)
    assert (status == St.BAD_INPUT).sum() == 3 + 4 + 5 + 6 and (status == St.OK).sum() == 6
    _, _, status = run_grid(world, "table end", "earth", "moon", "sun", 3, 5, dep0_ns=EPOCH0_NS - 30 * DAY, dep_step_ns=25 * DAY, tof0_ns=10 * DAY, tof_step_ns=10 * DAY)
    assert (status == St.EPHEM_RANGE).any() and (status == St.OK).any() and (status[0] == St.EPHEM_RANGE).all()
    empty = world["ctx"].lambert_grid(world["earth"], world["moon"], world["sun"], [P.C3], 0, 3, dep0_ns=EPOCH0_NS, dep_step_ns=DAY, tof0_ns=DAY, tof_step_ns=DAY)
    assert empty.values.shape == (1, 0, 3) and empty.status.shape == (0, 3) and empty.best(P.C3) is None
    with pytest.raises(ValueError, match="radius zero"):
        lambert.grid_definition(world["sun"], world["moon"], world["sun"], world["almanac"], world["central"], 1, 1, EPOCH0_NS, DAY, tof0_ns=DAY, tof_step_ns=DAY)
    with pytest.raises(RuntimeError, match="the departure body's chain is the centre's"):
        world["ctx"].lambert_grid(world["sun"], world["moon"], world["sun"], [P.C3], 1, 1, dep0_ns=EPOCH0_NS, dep_step_ns=DAY, tof0_ns=DAY, tof_step_ns=DAY)


def test_7_device_pointers_on_a_stream_equal_the_host_flavour(world):
    import torch
    ctx, lib, dev = world["ctx"], _abi.load_library(), torch.device("cuda", 0)
    params = [P.C3, P.X, P.V2Z]
    rv1, rv2, tof = BATCH
    host = ctx.lambert_batch(rv1, rv2, tof, MU_EARTH, params, Way.LongWay)
    q = _abi.LambertQuery()
    ctx._lambert_query(q, [int(p) for p in params], Way.LongWay, 0, 0, 1e-4, 1000)
    d1, d2, dt = (torch.from_numpy(a).to(dev) for a in (rv1, rv2, tof))
    guard = 64
    values = torch.full((3 * 70 + guard,), 12345.0, dtype=torch.float64, device=dev)
    status = torch.full((70 + guard,), -7, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        rc = lib.nyx_hip_lambert_batch_device(ctx._h, C.c_void_p(d1.data_ptr()), C.c_void_p(d2.data_ptr()), C.c_void_p(dt.data_ptr()), 70, MU_EARTH, C.byref(q),
                                              C.c_void_p(values.data_ptr()), C.c_void_p(status.data_ptr()), C.c_void_p(stream.cuda_stream))
    assert rc == 0, _abi.last_error()
    stream.synchronize()
    v, s = values.cpu().numpy(), status.cpu().numpy()
    np.testing.assert_array_equal(v[:210].reshape(3, 70).view(np.uint64), host.values.view(np.uint64))
    np.testing.assert_array_equal(s[:70], host.status)
    assert (v[210:] == 12345.0).all() and (s[70:] == -7).all()
    # the grid: 5 x 70 of test_3, the raw query the Python entry builds
    kw = dict(dep0_ns=EPOCH0_NS + DAY // 2, dep_step_ns=DAY, arr0_ns=EPOCH0_NS + 10 * DAY, arr_step_ns=2 * DAY // 5)
    hostg = ctx.lambert_grid(world["earth"], world["jupiter"], world["sun"], params, 5, 70, **kw)
    g = _abi.LambertGridQuery()
    ctx._lambert_query(g.solve, [int(p) for p in params], Way.Auto, 0, 0, 1e-4, 1000)
    for dst, body in ((g.dep, "earth"), (g.arr, "jupiter"), (g.centre, "sun")):
        chain = lambert.check_chain(body, world[body].naif_id, world["almanac"], world["central"])
        dst.n_chain = len(chain)
        for k, (seg, sign) in enumerate(chain):
            dst.chain_segment[k], dst.chain_sign[k] = seg, sign
    g.n_dep, g.n_arr, g.dep0_ns, g.dep_step_ns, g.arr0_ns, g.arr_step_ns, g.mu_km3_s2 = 5, 70, kw["dep0_ns"], kw["dep_step_ns"], kw["arr0_ns"], kw["arr_step_ns"], float(world["sun"].mu_km3_s2)
    values = torch.full((3 * 350 + guard,), 12345.0, dtype=torch.float64, device=dev)
    status = torch.full((350 + guard,), -7, dtype=torch.int32, device=dev)
    with torch.cuda.stream(stream):
        rc = lib.nyx_hip_lambert_grid_device(ctx._h, C.byref(g), C.c_void_p(values.data_ptr()), C.c_void_p(status.data_ptr()), C.c_void_p(stream.cuda_stream))
    assert rc == 0, _abi.last_error()
    stream.synchronize()
    v, s = values.cpu().numpy(), status.cpu().numpy()
    np.testing.assert_array_equal(v[:1050].reshape(3, 5, 70).view(np.uint64), hostg.values.view(np.uint64))
    np.testing.assert_array_equal(s[:350].reshape(5, 70), hostg.status)
    assert (v[1050:] == 12345.0).all() and (s[350:] == -7).all()
    # a context with an integration-frame swap is refused, nothing launched
    swapped = nx.GpuContext(world["prop"].compile(world["almanac"], world["central"], state_frame=world["moon"]))
    try:
        with pytest.raises(RuntimeError, match="integration-frame swap"):
            swapped.lambert_grid(world["earth"], world["jupiter"], world["sun"], params, 5, 70, **kw)
    finally:
        swapped.close()
