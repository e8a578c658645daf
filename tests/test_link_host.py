"""CPU: the definition of the link report (nyx_amd/links.py) against checks that do not share its formulas.

* Visible against a brute-force scan of the segment between the two spacecraft: 20001 points against the sphere, for 400 random
  pairs about a body of radius 1; pairs whose line passes within 1e-3 of the limb are left out (fewer than 5 %, asserted).  A scan of
  20001 points over at most 8 units of length misses the closest point by at most 2e-4 along the line, that is by about
  (2e-4)^2 / 2 = 2e-8 in distance: far inside the 1e-3 left out.
* RangeRate against a centred difference of Range along two-body arcs.  The states h = 0.01 s before and after come from one
  classical RK4 step each (error O(h^5): nothing); the centred difference has a truncation error of h^2 / 6 |range'''|, and with w
  the relative speed, a <= 0.02 km/s^2 the relative acceleration and j <= 1e-4 km/s^3 its rate, |range'''| <= 3 w^3 / range^2 +
  3 w a / range + j (differentiate range^2 = rho . rho three times); its rounding error is 2 x 2^-53 x 2e4 km / 0.02 s ~ 2e-10
  km/s, allowed as 1e-9.  The bound is formed per pair: the orbits meet head-on, and a pair 200 km apart bends its range fast.
* Visible <=> BodyClearance > 0 whenever 0 <= tau <= 1.
* Hand cases: opposite sides, same side, a tangent line +- 1e-9 relative, coincident states, no body, two bodies of which the second
  obstructs.
* ReferenceDoppler differs from RangeRate by rho . v_tx / |rho| (to the rounding of three divisions)."""
import numpy as np
import pytest

import nyx_amd as nx
from nyx_amd import ephem, links
from nyx_amd.links import LinkParameter as L
from scenarios import EPOCH0_NS, leo_full_setup, leo_nominal

UNIT = nx.Frame(nx.EARTH, 1.0, 1.0)          # a centre of radius 1: no almanac needed
MU = ephem.MU_EARTH


def value(p, rx, tx, bodies=(UNIT,), central=UNIT, almanac=None, body=None, epoch=EPOCH0_NS):
    return links.link_value(p, rx, tx, epoch, None if bodies is None else list(bodies), almanac, central, body=body)


def rv(r, v=(0.0, 0.0, 0.0)):
    return np.concatenate([np.asarray(r, dtype=np.float64), np.asarray(v, dtype=np.float64)])


def random_pairs(n, seed):
    rng = np.random.default_rng(seed)

    def points():
        d = rng.standard_normal((n, 3))
        return d / np.linalg.norm(d, axis=1)[:, None] * rng.uniform(1.2, 4.0, n)[:, None]

    return np.hstack([points(), rng.standard_normal((n, 3))]), np.hstack([points(), rng.standard_normal((n, 3))])


def test_visible_against_a_brute_force_scan_of_the_segment():
    rx, tx = random_pairs(400, seed=5)
    s = np.linspace(0.0, 1.0, 20001)[None, :, None]
    dist = np.linalg.norm(rx[:, None, :3] * (1.0 - s) + tx[:, None, :3] * s, axis=2).min(axis=1)
    clearance = value(L.BodyClearance, rx, tx, body=0)
    keep = np.abs(clearance - 0.0) >= 1e-3
    assert (~keep).mean() < 0.05
    blocked = dist <= 1.0
    assert 0.15 < blocked[keep].mean() < 0.85                              # both answers are well represented
    np.testing.assert_array_equal(value(L.Visible, rx, tx)[keep], np.where(blocked[keep], 0.0, 1.0))
    np.testing.assert_array_equal(value(L.BodyObstructs, rx, tx, body=UNIT)[keep], np.where(blocked[keep], 1.0, 0.0))
    np.testing.assert_array_equal(value(L.ObstructingBody, rx, tx)[keep], np.where(blocked[keep], 0.0, -1.0))
    # the clearance is the scan's closest distance less the radius wherever the closest point lies inside the segment
    inside = (dist < np.linalg.norm(rx[:, :3], axis=1) - 1e-6) & (dist < np.linalg.norm(tx[:, :3], axis=1) - 1e-6)
    assert inside.sum() > 100 and np.abs(clearance[inside] - (dist[inside] - 1.0)).max() < 1e-6
    np.testing.assert_array_equal(value(L.Clearance, rx, tx), clearance)   # one body: the minimum is its own


def _rk4(y, h):
    def f(y):
        r = y[..., :3]
        return np.concatenate([y[..., 3:], -MU * r / np.linalg.norm(r, axis=-1, keepdims=True) ** 3], axis=-1)

    k1 = f(y)
    k2 = f(y + 0.5 * h * k1)
    k3 = f(y + 0.5 * h * k2)
    k4 = f(y + h * k3)
    return y + h / 6.0 * (k1 + 2.0 * k2 + 2.0 * k3 + k4)


def test_range_rate_against_a_centred_difference_of_range_on_two_body_arcs():
    rng = np.random.default_rng(9)
    nominal = leo_nominal()
    rx = nominal + rng.standard_normal((64, 6)) * np.array([200.0, 200.0, 200.0, 0.2, 0.2, 0.2])
    tx = nominal * np.array([1, 1, 1, -1, -1, -1]) + rng.standard_normal((64, 6)) * np.array([200.0, 200.0, 200.0, 0.2, 0.2, 0.2])
    # along the arcs: a few minutes of coarse steps first, so that the pairs are not all near one geometry
    for k in range(64):
        for _ in range(k):
            rx[k], tx[k] = _rk4(rx[k], 10.0), _rk4(tx[k], 10.0)
    h = 0.01
    earth = leo_full_setup(degree=0)[2]
    diff = (value(L.Range, _rk4(rx, h), _rk4(tx, h), (earth,), earth) - value(L.Range, _rk4(rx, -h), _rk4(tx, -h), (earth,), earth)) / (2.0 * h)
    rate = value(L.RangeRate, rx, tx, (earth,), earth)
    assert np.abs(rate).max() > 5.0 and np.abs(rate).min() < 14.0            # head-on orbits: km/s of closing speed
    rho_km, w = value(L.Range, rx, tx, (earth,), earth), value(L.RelativeSpeed, rx, tx, (earth,), earth)
    bound = h * h / 6.0 * (3.0 * w ** 3 / rho_km ** 2 + 3.0 * w * 0.02 / rho_km + 1e-4) + 1e-9
    assert bound.max() < 1e-5 and np.median(bound) < 1e-7           # (what the bound comes to: tight for all but the closest pairs)
    assert (np.abs(rate - diff) <= bound).all(), (np.abs(rate - diff) / bound).max()
    # and the reference's Doppler differs from it by the transmitter's share
    rho = rx[:, :3] - tx[:, :3]
    rng_km = np.linalg.norm(rho, axis=1)
    a, b = np.abs((rho * rx[:, 3:]).sum(axis=1)) / rng_km, np.abs((rho * tx[:, 3:]).sum(axis=1)) / rng_km
    gap = value(L.ReferenceDoppler, rx, tx, (earth,), earth) - rate
    assert np.abs(b).max() > 1.0                                               # (the two are different numbers)
    assert (np.abs(gap - (rho * tx[:, 3:]).sum(axis=1) / rng_km) <= 16.0 * np.finfo(float).eps * (a + b)).all()
    speed = value(L.RelativeSpeed, rx, tx, (earth,), earth)
    assert (np.abs(rate) <= speed * (1.0 + 1e-15)).all() and np.allclose(speed, np.linalg.norm(rx[:, 3:] - tx[:, 3:], axis=1), rtol=1e-15)
    los = np.stack([value(p, rx, tx, (earth,), earth) for p in (L.LosX, L.LosY, L.LosZ)], axis=1)
    assert np.abs(np.linalg.norm(los, axis=1) - 1.0).max() < 4e-16 and np.allclose(los * rng_km[:, None], rho, rtol=1e-15)


def test_visible_is_a_positive_clearance_whenever_the_closest_point_lies_inside_the_segment():
    rx, tx = random_pairs(2000, seed=21)
    tau, d2, obstructs, clearance = links.sight(rx[:, :3], tx[:, :3], np.zeros(3), 1.0)
    inside = (tau >= 0.0) & (tau <= 1.0)
    assert 200 < inside.sum() < 1900
    np.testing.assert_array_equal(~obstructs[inside], clearance[inside] > 0.0)
    assert not obstructs[~inside].any()                                        # the closest point is an end of the segment: a spacecraft
    np.testing.assert_array_equal(value(L.Visible, rx, tx) == 1.0, ~obstructs)


def test_hand_cases():
    # opposite sides of the body: obstructed, by the whole radius
    assert value(L.Visible, rv([2, 0, 0]), rv([-2, 0, 0])) == 0.0 and value(L.Clearance, rv([2, 0, 0]), rv([-2, 0, 0])) == -1.0
    assert value(L.ObstructingBody, rv([2, 0, 0]), rv([-2, 0, 0])) == 0.0
    # the same side: visible, and the clearance is that of the nearer spacecraft
    assert value(L.Visible, rv([2, 0, 0]), rv([3, 0.5, 0])) == 1.0 and value(L.Clearance, rv([2, 0, 0]), rv([3, 0.5, 0])) == 1.0
    assert value(L.ObstructingBody, rv([2, 0, 0]), rv([3, 0.5, 0])) == -1.0
    # a line tangent to the sphere, moved in and out by 1e-9 of the radius
    for eps, seen in ((1e-9, 1.0), (-1e-9, 0.0)):
        a, b = rv([-3.0, 1.0 + eps, 0.0]), rv([5.0, 1.0 + eps, 0.0])
        assert value(L.Visible, a, b) == seen and abs(value(L.BodyClearance, a, b, body=0) - eps) < 1e-15
    # coincident spacecraft: tau is NaN - not obstructed, no clearance, no rate, no direction; the range and the speed exist
    p = rv([2, 0, 0], [0, 1, 0])
    assert value(L.Visible, p, p) == 1.0 and value(L.ObstructingBody, p, p) == -1.0 and value(L.BodyObstructs, p, p, body=0) == 0.0
    assert np.isnan(value(L.BodyClearance, p, p, body=0)) and value(L.Clearance, p, p) == np.inf      # (a NaN never wins the minimum)
    assert np.isnan(value(L.RangeRate, p, p)) and np.isnan(value(L.ReferenceDoppler, p, p)) and np.isnan(value(L.LosX, p, p))
    assert value(L.Range, p, p) == 0.0 and value(L.RelativeSpeed, p, p) == 0.0
    # no body at all
    assert value(L.Visible, rv([2, 0, 0]), rv([-2, 0, 0]), bodies=()) == 1.0 and value(L.ObstructingBody, rv([2, 0, 0]), rv([-2, 0, 0]), bodies=()) == -1.0
    assert value(L.Clearance, rv([2, 0, 0]), rv([-2, 0, 0]), bodies=()) == np.inf
    with pytest.raises(ValueError, match="names no body"):
        links.link_param((L.BodyClearance, 0), [])
    # exact values: a 3-4-5 geometry
    a, b = rv([3, 0, 0], [0, 1, 0]), rv([0, 4, 0], [1, 0, 0])
    assert value(L.Range, a, b) == 5.0 and value(L.RangeRate, a, b) == (3 * -1 + -4 * 1) / 5.0 and value(L.ReferenceDoppler, a, b) == -4.0 / 5.0
    assert (value(L.LosX, a, b), value(L.LosY, a, b), value(L.LosZ, a, b)) == (3.0 / 5.0, -4.0 / 5.0, 0.0)
    assert value(L.RelativeSpeed, a, b) == np.sqrt(2.0) and value(L.Visible, a, b) == 1.0 and abs(value(L.Clearance, a, b) - 1.4) < 1e-15


def test_two_bodies_of_which_the_second_obstructs():
    """The Earth and the Moon of the almanac of the tests: a line through the Moon's centre, far from the Earth."""
    _, almanac, earth = leo_full_setup(degree=0)
    moon = almanac.frame_info(nx.MOON)
    from nyx_amd.eclipse import body_position
    pm = body_position(nx.MOON, np.int64(EPOCH0_NS), almanac, earth)
    side = np.cross(pm, [0.0, 0.0, 1.0])
    side = side / np.linalg.norm(side) * 5000.0
    a, b = rv(pm + side), rv(pm - side)
    both = (earth, moon)
    assert value(L.Visible, a, b, both, earth, almanac) == 0.0 and value(L.ObstructingBody, a, b, both, earth, almanac) == 1.0
    assert value(L.BodyObstructs, a, b, both, earth, almanac, body=earth) == 0.0 and value(L.BodyObstructs, a, b, both, earth, almanac, body=moon) == 1.0
    assert abs(value(L.BodyClearance, a, b, both, earth, almanac, body=1) + moon.mean_equatorial_radius_km) < 1e-6
    assert value(L.Clearance, a, b, both, earth, almanac) == value(L.BodyClearance, a, b, both, earth, almanac, body=1)
    assert value(L.BodyClearance, a, b, both, earth, almanac, body=0) > 3e5
    # the order of the bodies decides the index, not the answer
    assert value(L.ObstructingBody, a, b, (moon, earth), earth, almanac) == 0.0
    # the Earth alone (the default): visible
    assert value(L.Visible, a, b, None, earth, almanac) == 1.0 and links.link_value(L.Visible, a, b, EPOCH0_NS, None, None, earth) == 1.0
    # an epoch outside the Moon's ephemerides: NaN for what needs the Moon, and the helper says so
    late = np.int64(EPOCH0_NS + 400 * 86400 * nx.NS_PER_S)
    assert np.isnan(value(L.Visible, a, b, both, earth, almanac, epoch=late)) and abs(value(L.Range, a, b, both, earth, almanac, epoch=late) - 10000.0) < 1e-9
    assert links.outside_ephemerides(np.array([EPOCH0_NS, late]), both, almanac, earth).tolist() == [False, True]
    assert not links.outside_ephemerides(np.array([late]), None, None, earth).any()


def test_what_the_python_layer_refuses_of_the_bodies():
    _, almanac, earth = leo_full_setup(degree=0)
    moon = almanac.frame_info(nx.MOON)
    links.check_link_bodies([], None, earth)
    links.check_link_bodies([earth], None, earth)
    with pytest.raises(ValueError, match="needs an almanac"):
        links.check_link_bodies([earth, moon], None, earth)
    with pytest.raises(ValueError, match="9 bodies, 0 .. 8"):
        links.check_link_bodies([earth] * 9, almanac, earth)
    with pytest.raises(ValueError, match=r"bodies\[1\] needs a finite mean radius > 0"):
        links.check_link_bodies([earth, nx.Frame(nx.MOON, 4902.8, 0.0)], almanac, earth)
    with pytest.raises(KeyError, match="planetary data"):
        links.check_link_bodies([nx.Frame(499, 42828.0, 3396.0)], almanac, earth)
    with pytest.raises(TypeError, match="not a LinkParameter"):
        links.link_param(nx.StateParameter.Rmag, [earth])
    with pytest.raises(ValueError, match="per-body parameter"):
        links.link_param(L.BodyClearance, [earth])
    with pytest.raises(ValueError, match="takes no body"):
        links.link_param((L.Range, 0), [earth])
    assert links.link_param((L.BodyObstructs, moon), [earth, moon]) == (L.BodyObstructs, 1) and links.link_param(L.Range) == (L.Range, 0)
    assert [int(p) for p in L] == list(range(12)) and links.PER_BODY == {L.BodyClearance, L.BodyObstructs}
