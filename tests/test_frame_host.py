"""CPU: the host definition of the encounter report (nyx_amd/frames.py), which the device kernel (csrc/frame_kernel.hip) is tested against.

* POSITION: `frames.body_state(...)[0]` equals the oracle's `nyx_oracle_body_position` BIT FOR BIT for the Moon (a chain of two), the
  Sun and Jupiter (chains of three) at 64 epochs over the span of the almanac, the exact end of coverage among them.
* VELOCITY: the oracle exports no body velocity, so it is pinned on an INDEPENDENT algorithm - numpy's `chebder` + `chebval` on the
  record's coefficients, divided by the record's radius, summed along the chain - within 256 eps sum_j j^2 |c_j| / radius over the
  chain's records (the error of a Clenshaw derivative of degree n <= 16 is of order n eps sum j^2 |c_j|: an order of magnitude of
  room; a wrong recurrence or a missing 1 / radius is off by the value itself), and cross-checked against a centred difference of the
  oracle's positions at +-32 s inside one record to 1e-8 km/s (rounding eps |r| / h ~ 1e-9 km/s for the Sun, truncation
  h^2 / 6 w^2 v ~ 1.2e-9 km/s for the Moon).
* identity and round trip of `to_frame`; the B-plane against the reference-held Davis vector (tests/golden/bplane_davis.json); NaN
  for the hyperbola-only codes of a LEO state; the names a parameter can be given by; the refusals of a target."""
import ctypes as C
import json
import os

import numpy as np
import pytest
from numpy.polynomial import chebyshev

import nyx_amd as nx
import oracle_lib
from nyx_amd import _abi, eclipse, ephem, frames
from nyx_amd.frames import FrameParameter as F
from scenarios import EPOCH0_NS, leo_full_setup, leo_nominal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
BODIES = (nx.MOON, nx.SUN, nx.JUPITER_BARYCENTER)


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def world():
    prop, almanac, central = leo_full_setup(degree=0, point_masses=BODIES)
    compiled = prop.compile(almanac, central)
    index = {int(compiled.cfg.bodies[b].naif_id): b for b in range(compiled.cfg.n_bodies)}
    # the segments end at different epochs: the span of a body is that of the segment of its chain that ends first, and 64 epochs
    # over it - its first instant, the exact end of its coverage, one off the whole second - are asked of every body
    epochs, end_ns = {}, {}
    for naif in BODIES:
        segs = [almanac.segments[s] for s, _ in eclipse.body_chain(naif, almanac, central)]
        t0 = max(float(s.init_et_s) for s in segs)
        t1 = min(float(s.init_et_s) + float(s.interval_s) * s.records.shape[0] for s in segs)
        end_ns[naif] = int(round(t1 * 1e9))
        assert nx.to_seconds(end_ns[naif]) == t1
        epochs[naif] = np.concatenate([np.linspace(int(np.ceil(t0 * 1e9)), end_ns[naif], 63).astype(np.int64), [end_ns[naif]]])
        epochs[naif][-2] = EPOCH0_NS + 5400 * 10**9 + 123456789
    return dict(compiled=compiled, almanac=almanac, central=central, lib=oracle_lib.load(), index=index, epochs=epochs, end_ns=end_ns)


def oracle_position(w, naif, epoch_ns):
    pos, st = np.zeros(3), C.c_int32()
    w["lib"].nyx_oracle_body_position(C.byref(w["compiled"].cfg), w["index"][naif], int(epoch_ns), pos.ctypes.data_as(_abi.c_double_p), C.byref(st))
    return pos, st.value


def test_positions_are_the_oracles_bit_for_bit(world):
    w = world
    assert [len(eclipse.body_chain(b, w["almanac"], w["central"])) for b in BODIES] == [2, 3, 3]
    for naif in BODIES:
        epochs = w["epochs"][naif]
        assert len(epochs) == 64 and epochs[-1] == w["end_ns"][naif]
        got = frames.body_state(naif, epochs, w["almanac"], w["central"])[0]
        for k, ep in enumerate(epochs):
            pos, st = oracle_position(w, naif, ep)
            assert st == 0, (naif, ep)
            assert (bits(got[k]) == bits(pos)).all(), (naif, ep, got[k], pos)
        # and the value of cheby_state is that of eclipse.cheby_position
        for seg, _ in eclipse.body_chain(naif, w["almanac"], w["central"]):
            s = w["almanac"].segments[seg]
            et = frames._ns_to_seconds(epochs)
            assert (bits(frames.cheby_state(s, et)[0]) == bits(eclipse.cheby_position(s, et))).all()
    # one nanosecond past the end of coverage, and far outside: the oracle's status, NaN here; the centre (no chain) is everywhere
    far = np.array([w["end_ns"][nx.MOON] + 10**9, EPOCH0_NS - 400 * 86400 * 10**9], dtype=np.int64)
    for ep in far:
        assert oracle_position(w, nx.MOON, ep)[1] == _abi.ERR_EPHEM_RANGE
    r, v = frames.body_state(nx.MOON, far, w["almanac"], w["central"])
    assert np.isnan(r).all() and np.isnan(v).all()
    r, v = frames.body_state(nx.EARTH, far, w["almanac"], w["central"])
    assert (r == 0.0).all() and (v == 0.0).all()


def independent_velocity(w, naif, epoch_ns):
    """(v[3], bound[3]) by numpy's Chebyshev derivative, record by record along the chain."""
    et = float(frames._ns_to_seconds(np.int64(epoch_ns)))
    v, bound = np.zeros(3), np.zeros(3)
    for seg_i, sign in eclipse.body_chain(naif, w["almanac"], w["central"]):
        seg = w["almanac"].segments[seg_i]
        rec_all = np.asarray(seg.records, dtype=np.float64)
        idx = min(int(np.floor((et - float(seg.init_et_s)) / float(seg.interval_s))), len(rec_all) - 1)
        rec, nc = rec_all[idx], seg.n_coeffs
        t = (et - rec[0]) / rec[1]
        assert -1.0 - 1e-9 <= t <= 1.0 + 1e-9
        for c in range(3):
            cf = rec[2 + c * nc:2 + (c + 1) * nc]
            v[c] += sign * chebyshev.chebval(t, chebyshev.chebder(cf)) / rec[1]
            bound[c] += 256.0 * EPS * np.sum(np.arange(nc) ** 2 * np.abs(cf)) / rec[1]
    return v, bound


def test_velocities_against_an_independent_derivative(world):
    w = world
    worst = 0.0
    for naif in BODIES:
        got = frames.body_state(naif, w["epochs"][naif], w["almanac"], w["central"])[1]
        for k, ep in enumerate(w["epochs"][naif]):
            want, bound = independent_velocity(w, naif, ep)
            err = np.abs(got[k] - want)
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all(), (naif, ep, got[k], want, bound)
            assert np.linalg.norm(want) > 1e-3          # (a missing term would be off by the value itself: km/s, not 1e-12)
    print(f"velocity: worst error / bound = {worst:.3f}")


def test_velocities_against_a_centred_difference_of_the_oracles_positions(world):
    w = world
    h = 32 * 10**9
    worst = 0.0
    for naif in BODIES:
        checked = 0
        for ep in w["epochs"][naif][1:-2:4]:
            # inside one record of every segment of the chain: the centred difference must not straddle a record seam
            et = float(frames._ns_to_seconds(np.int64(ep)))
            inside = True
            for seg_i, _ in eclipse.body_chain(naif, w["almanac"], w["central"]):
                s = w["almanac"].segments[seg_i]
                f = ((et - float(s.init_et_s)) / float(s.interval_s)) % 1.0 * float(s.interval_s)
                inside &= 40.0 < f < float(s.interval_s) - 40.0
            if not inside:
                continue
            plus, st1 = oracle_position(w, naif, ep + h)
            minus, st2 = oracle_position(w, naif, ep - h)
            assert st1 == st2 == 0
            fd = (plus - minus) / 64.0
            got = frames.body_state(naif, np.int64(ep), w["almanac"], w["central"])[1]
            worst = max(worst, float(np.abs(got - fd).max()))
            assert np.abs(got - fd).max() <= 1e-8, (naif, ep, got, fd)
            checked += 1
        assert checked >= 12, (naif, checked)
    print(f"velocity vs centred difference: worst {worst:.3e} km/s")


def test_identity_and_round_trip(world):
    w = world
    rng = np.random.default_rng(5)
    rv = leo_nominal()[None, :] + rng.standard_normal((64, 6)) * np.array([100.0, 100.0, 100.0, 0.1, 0.1, 0.1])
    rv[0, 2] = -0.0
    same = frames.to_frame(rv, w["epochs"][nx.MOON], w["central"], w["almanac"], w["central"])
    assert same is not rv and (bits(same) == bits(rv)).all()
    for naif in BODIES:
        target = w["almanac"].frame_info(naif)
        moved = frames.to_frame(rv, w["epochs"][naif], target, w["almanac"], w["central"])
        r, v = frames.body_state(naif, w["epochs"][naif], w["almanac"], w["central"])
        body = np.concatenate([r, v], axis=-1)
        assert (bits(moved) == bits(rv - body)).all()
        back = moved + body
        # one rounding of the difference and one of the sum, each half an ulp of its result, which is no larger than the larger operand
        ulp = np.spacing(np.maximum(np.abs(rv), np.maximum(np.abs(body), np.abs(moved))))
        assert (np.abs(back - rv) <= ulp).all(), np.abs(back - rv).max()
    out = frames.to_frame(rv[:2], np.array([w["end_ns"][nx.MOON] + 10**9, EPOCH0_NS], dtype=np.int64), w["almanac"].frame_info(nx.MOON), w["almanac"], w["central"])
    assert np.isnan(out[0]).all() and np.isfinite(out[1]).all()


def test_the_b_plane_of_the_reference_held_vector():
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "bplane_davis.json")))
    rv = np.array(g["state_km_km_s"])
    val = {p: float(frames.state_frame_value(p, rv, ephem.MU_EARTH)) for p in F}
    assert g["tolerance_km"] == 1e-5
    assert abs(val[F.BdotT] - g["b_dot_t_km"]) < 1e-5 and abs(val[F.BdotR] - g["b_dot_r_km"]) < 1e-5, (val[F.BdotT], val[F.BdotR])
    assert val[F.BMagnitude] == np.sqrt(val[F.BdotT] ** 2 + val[F.BdotR] ** 2)
    assert abs(val[F.BAngle] - np.degrees(np.arctan2(val[F.BdotR], val[F.BdotT]))) <= 2 * np.spacing(val[F.BAngle]) and -180.0 < val[F.BAngle] <= 180.0
    assert val[F.VInfinity] == np.sqrt(val[F.C3]) and abs(val[F.VInfinity] ** 2 - val[F.C3]) <= 4 * np.spacing(val[F.C3])
    assert val[F.C3] == 2.0 * val[F.Energy] or abs(val[F.C3] - 2.0 * val[F.Energy]) <= 8 * np.spacing(val[F.C3])
    assert val[F.Eccentricity] > 1.0 and val[F.SemiMajorAxis] < 0.0
    # B lies in the plane normal to the incoming asymptote and has the semi-minor axis for its length
    b = abs(val[F.SemiMajorAxis]) * np.sqrt(val[F.Eccentricity] ** 2 - 1.0)
    assert abs(val[F.BMagnitude] - b) <= 1e-9 * b
    # the wrap of the angle: a B vector along -T with BdotR = -0 is at +180
    assert float(np.where(frames._atan2(-0.0, -1.0) * frames._TO_DEG == -180.0, 180.0, 0.0)) == 180.0


def test_a_state_that_is_not_hyperbolic(world):
    w = world
    rv = leo_nominal()
    for p in F:
        v = float(frames.frame_value(p, rv, EPOCH0_NS, w["central"], w["almanac"], w["central"]))
        assert np.isnan(v) == (p in frames.HYPERBOLA_ONLY), (p, v)
    assert len(frames.HYPERBOLA_ONLY) == 5 and len(F) == 25
    # an array of both kinds: the LEO row NaN, the hyperbolic row finite, the others unaffected
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "bplane_davis.json")))
    both = np.array([rv, g["state_km_km_s"]])
    bt = frames.state_frame_value(F.BdotT, both, ephem.MU_EARTH)
    assert np.isnan(bt[0]) and abs(bt[1] - g["b_dot_t_km"]) < 1e-5
    assert np.isfinite(frames.state_frame_value(F.C3, both, ephem.MU_EARTH)).all()


def test_the_names_of_a_parameter_and_the_refusals_of_a_target(world):
    w = world
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "bplane_davis.json")))
    both = np.array([leo_nominal(), g["state_km_km_s"]])
    # the B-plane of a state about its own centre: the same function, NaN when not hyperbolic
    bt, br = nx.params.bplane_of_state(both, ephem.MU_EARTH)
    assert (bits(bt) == bits(frames.frame_value(F.BdotT, both, EPOCH0_NS, w["central"], w["almanac"], w["central"]))).all()
    assert (bits(br) == bits(frames.frame_value(F.BdotR, both, EPOCH0_NS, w["central"], w["almanac"], w["central"]))).all()
    assert np.isnan(bt[0]) and np.isnan(br[0]) and np.isfinite(bt[1]) and np.isfinite(br[1])
    assert "BLTOF" not in F.__members__
    # the names a FrameParameter can be given by
    assert frames.frame_param(nx.StateParameter.Rmag) is F.Rmag and frames.frame_param(19) is F.C3 and frames.frame_param(F.BAngle) is F.BAngle
    for bad in (nx.StateParameter.Cr, nx.StateParameter.Isp, "Rmag", True):
        with pytest.raises(TypeError):
            frames.frame_param(bad)
    with pytest.raises(ValueError):
        frames.frame_param(25)
    # a target the almanac cannot reach, or without a mu
    with pytest.raises(KeyError, match="planetary data"):
        frames.frame_value(F.Rmag, both, EPOCH0_NS, nx.Frame(499, 42828.0), w["almanac"], w["central"])
    with pytest.raises(ValueError, match="finite mu"):
        frames.frame_value(F.Rmag, both, EPOCH0_NS, nx.Frame(nx.MOON, 0.0), w["almanac"], w["central"])
