"""The host definition of the Lambert transfers (nyx_amd/lambert.py) on the CPU: the reference's own unit-test vectors (Vallado 7-1,
tests/golden/lambert_vallado.json), every solution FLOWN to its target by a two-body step written here, the way rule, every status from
a hand-made input, and the series window of the time equation."""
import json
import math
import os

import numpy as np
import pytest

import nyx_amd as nx
from nyx_amd import lambert
from nyx_amd.lambert import LambertParameter as P, LambertStatus as St, TransferKind as Way

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lambert_vallado.json")))
MU = GOLDEN["mu_km3_s2"]


def stumpff(z):
    if z > 1e-6:
        s = math.sqrt(z)
        return (1.0 - math.cos(s)) / z, (s - math.sin(s)) / (s * s * s)
    if z < -1e-6:
        s = math.sqrt(-z)
        return (math.cosh(s) - 1.0) / -z, (math.sinh(s) - s) / (s * s * s)
    return 0.5 - z / 24.0, 1.0 / 6.0 - z / 120.0


def kepler_step(r0, v0, dt, mu):
    """The two-body state after dt by the universal variable (Curtis, Orbital Mechanics, algorithms 3.3 and 3.4): the universal Kepler
    equation is monotone in chi (its derivative is the radius), solved by Newton's method kept inside a bracket."""
    r0, v0 = np.asarray(r0, dtype=float), np.asarray(v0, dtype=float)
    rn, sq = np.linalg.norm(r0), math.sqrt(mu)
    vr = float(r0 @ v0) / rn
    alpha = 2.0 / rn - float(v0 @ v0) / mu

    def f(chi):
        c, s = stumpff(alpha * chi * chi)
        val = rn * vr / sq * chi * chi * c + (1.0 - alpha * rn) * chi ** 3 * s + rn * chi - sq * dt
        der = rn * vr / sq * chi * (1.0 - alpha * chi * chi * s) + (1.0 - alpha * rn) * chi * chi * c + rn
        return val, der

    lo, hi = 0.0, sq * dt / rn
    while f(hi)[0] < 0.0:
        lo, hi = hi, 2.0 * hi
    chi = 0.5 * (lo + hi)
    for _ in range(200):
        val, der = f(chi)
        lo, hi = (chi, hi) if val < 0.0 else (lo, chi)
        new = chi - val / der
        if not lo < new < hi:
            new = 0.5 * (lo + hi)
        if abs(new - chi) <= 1e-15 * abs(chi):
            chi = new
            break
        chi = new
    c, s = stumpff(alpha * chi * chi)
    fg, g = 1.0 - chi * chi / rn * c, dt - chi ** 3 / sq * s
    r = fg * r0 + g * v0
    rr = np.linalg.norm(r)
    fdot, gdot = sq / (rr * rn) * (alpha * chi ** 3 * s - chi), 1.0 - chi * chi / rr * c
    return r, fdot * r0 + gdot * v0


def flown(r1, r2, tof, status, values):
    """(relative arrival miss, relative arrival-velocity difference) of a solved problem"""
    assert status == St.OK
    r, v = kepler_step(r1, values[0:3], tof, MU)
    scale_v = max(np.linalg.norm(values[0:3]), np.linalg.norm(values[3:6]))
    return np.linalg.norm(r - r2) / np.linalg.norm(r2), np.linalg.norm(v - values[3:6]) / scale_v


def test_the_kepler_step_of_this_file_closes_an_orbit_and_keeps_its_energy():
    r0, v0 = np.array([7000.0, 100.0, -50.0]), np.array([0.3, 7.0, 2.5])
    a = 1.0 / (2.0 / np.linalg.norm(r0) - v0 @ v0 / MU)
    period = 2.0 * math.pi * math.sqrt(a ** 3 / MU)
    r, v = kepler_step(r0, v0, 3.0 * period, MU)
    assert np.linalg.norm(r - r0) < 1e-6 and np.linalg.norm(v - v0) < 1e-9
    r, v = kepler_step(r0, 2.0 * v0, 5000.0, MU)   # a hyperbola
    assert abs((v @ v / 2 - MU / np.linalg.norm(r)) / (2.0 * v0 @ v0 - MU / np.linalg.norm(r0)) - 1.0) < 1e-12
    np.testing.assert_allclose(np.cross(r, v), np.cross(r0, 2.0 * v0), rtol=1e-12)


def test_vallado_7_1_the_vectors_of_the_references_unit_tests():
    g = GOLDEN
    for way, key in ((Way.ShortWay, "short_way"), (Way.LongWay, "long_way")):
        sol = lambert.izzo(g["r_init_km"], g["r_final_km"], g["tof_s"], MU, way)
        assert np.linalg.norm(sol.v_init_km_s - g[key]["v_init_km_s"]) < g["velocity_tolerance_km_s"]
        assert np.linalg.norm(sol.v_final_km_s - g[key]["v_final_km_s"]) < g["velocity_tolerance_km_s"]
        assert abs(sol.v_inf_outgoing_right_ascension_deg() - g[key]["right_ascension_deg"]) < g["right_ascension_tolerance_deg"]
        assert abs(sol.v_inf_outgoing_declination_deg() - g["declination_deg"]) < g["declination_tolerance_deg"]
        # the accessors of the reference's LambertSolution, with its signs
        np.testing.assert_array_equal(sol.v_inf_outgoing_km_s(), -sol.v_init_km_s)
        np.testing.assert_array_equal(sol.v_inf_incoming_km_s(), -sol.v_final_km_s)
        assert sol.c3_km2_s2() == sol.of(P.C3) == pytest.approx(float(sol.v_init_km_s @ sol.v_init_km_s), rel=1e-15)
        np.testing.assert_array_equal(sol.transfer_orbit(), np.concatenate([g["r_init_km"], sol.v_init_km_s]))
        np.testing.assert_array_equal(sol.arrival_orbit(), np.concatenate([g["r_final_km"], sol.v_final_km_s]))
        assert sol.status == St.OK and sol.iterations >= 1 and sol.phi_rad == 0.0
    assert nx.izzo is lambert.izzo and nx.TransferKind is Way and nx.LambertParameter is P


def geometries():
    """The reference's three direction-regression geometries and 200 seeded ones, (r1 x r2).z < 0 in every other one."""
    out = [(np.array(g["r_init_km"]), np.array(g["r_final_km"]), g["tof_s"]) for g in GOLDEN["direction_geometries"]]
    rng = np.random.default_rng(7)
    for k in range(200):
        d1, d2 = rng.normal(size=3), rng.normal(size=3)
        r1, r2 = d1 / np.linalg.norm(d1) * rng.uniform(7000.0, 42000.0), d2 / np.linalg.norm(d2) * rng.uniform(7000.0, 42000.0)
        if (np.cross(r1, r2)[2] < 0.0) != (k % 2 == 0):
            r1, r2 = r1 * [1.0, -1.0, 1.0], r2 * [1.0, -1.0, 1.0]
        out.append((r1, r2, 10.0 ** rng.uniform(3.3, 5.5)))
    return out


def test_every_solution_flown_reaches_its_target():
    """All three ways, 0 to 2 revolutions, both paths, where feasible: the solution flown for tof_s reaches r2 within 1e-6 relative at
    the reference's tol = 1e-4 (a sweep of 3000 problems measured 1.0e-7), and arrives with v_final."""
    geo = geometries()
    assert sum(np.cross(r1, r2)[2] < 0.0 for r1, r2, _ in geo[3:]) == 100
    worst_r = worst_v = 0.0
    solved = {m: 0 for m in range(3)}
    for r1, r2, tof in geo:
        for way in Way:
            for m, hp in ((0, 0), (1, 0), (1, 1), (2, 0), (2, 1)):
                status, values, _ = lambert.solve(list(r1) + [0.0] * 3, list(r2) + [0.0] * 3, tof, MU, way, m, hp)
                if m > 0 and status == St.NOT_FEASIBLE:
                    continue
                dr, dv = flown(r1, r2, tof, status, values)
                worst_r, worst_v, solved[m] = max(worst_r, dr), max(worst_v, dv), solved[m] + 1
                assert dr < 1e-6, (r1, r2, tof, way, m, hp, dr)
                assert dv < 1e-6, (r1, r2, tof, way, m, hp, dv)
    print(f"worst relative arrival miss {worst_r:.2e}, arrival velocity {worst_v:.2e}; solved {solved}")
    assert solved[0] == 3 * len(geo) and solved[1] > 100 and solved[2] > 50


def test_auto_is_short_or_long_by_the_dnu_rule_and_the_normal_is_never_flipped():
    for r1, r2, tof in geometries():
        auto, short, long_ = (lambert.solve(list(r1) + [0.0] * 3, list(r2) + [0.0] * 3, tof, MU, w)[1] for w in Way)
        dnu = math.atan2(r2[1], r2[0]) - math.atan2(r1[1], r1[0])
        dnu += 2.0 * math.pi if dnu < 0.0 else 0.0
        np.testing.assert_array_equal(auto, long_ if dnu > math.pi else short)
        assert np.linalg.norm(short[0:3] - long_[0:3]) > 1e-3
        # the short way sweeps less than 180 deg about the natural normal r1 x r2, whatever the sign of its z
        assert short[P.TransferAngleDeg] < 180.0 < long_[P.TransferAngleDeg] and short[P.TransferAngleDeg] + long_[P.TransferAngleDeg] == pytest.approx(360.0)
        assert np.cross(r1, short[0:3]) @ np.cross(r1, r2) > 0.0 > np.cross(r1, long_[0:3]) @ np.cross(r1, r2)
    for g in GOLDEN["direction_geometries"]:
        if "auto" in g:
            assert (lambert.izzo(g["r_init_km"], g["r_final_km"], g["tof_s"], MU).of(P.TransferAngleDeg) > 180.0) == (g["auto"] == "long_way")


def test_every_status_from_a_hand_made_input():
    a, b = [7000.0, 0.0, 0.0, 0.0, 7.5, 0.0], [6000.0, 3000.0, 500.0, -3.0, 6.0, 1.0]
    cases = [(St.BAD_INPUT, ([math.nan] + a[1:], b, 3000.0), {}), (St.BAD_INPUT, (a, b[:5] + [math.inf], 3000.0), {}), (St.BAD_INPUT, ([0.0] * 6, b, 3000.0), {}),
             (St.BAD_INPUT, (a, [0.0] * 6, 3000.0), {}), (St.BAD_INPUT, (a, b, 0.0), {}), (St.BAD_INPUT, (a, b, -1.0), {}), (St.BAD_INPUT, (a, b, math.nan), {}),
             (St.DEGENERATE, (a, a, 3000.0), {}), (St.DEGENERATE, (a, [14000.0, 0.0, 0.0, 0.0, 0.0, 0.0], 3000.0), {}),
             (St.DEGENERATE, (a, [-7000.0, 0.0, 0.0, 0.0, 0.0, 0.0], 3000.0), {}),
             (St.NOT_FEASIBLE, (a, b, 3000.0), dict(n_revs=1)), (St.NOT_FEASIBLE, (a, b, 40000.0), dict(n_revs=255)),
             (St.TOO_CLOSE, (a, b, 1e-3), {}), (St.MAX_ITER, (a, b, 3000.0), dict(max_iter=1)), (St.OK, (a, b, 3000.0), {}), (St.OK, (a, b, 40000.0), dict(n_revs=2, high_path=1))]
    for want, (rv1, rv2, tof), kw in cases:
        status, values, extras = lambert.solve(rv1, rv2, tof, MU, Way.ShortWay, **kw)
        assert status == want, (want, rv1, rv2, tof, kw)
        assert np.isnan(values).all() if want != St.OK else np.isfinite(values).all()
        if want != St.OK:
            with pytest.raises(ValueError, match=want.name):
                lambert.izzo(rv1, rv2, tof, MU, Way.ShortWay, **kw)
    assert [int(s) for s in St] == list(range(7)) and St.EPHEM_RANGE == 6   # (the grid's own: tests/test_gpu_lambert.py)
    for bad in (dict(tol=1e-1), dict(tol=1e-14), dict(tol=math.nan), dict(max_iter=0), dict(max_iter=1001), dict(n_revs=-1), dict(n_revs=256), dict(high_path=2)):
        with pytest.raises(ValueError):
            lambert.izzo(a, b, 3000.0, MU, **bad)
    with pytest.raises(ValueError):
        lambert.izzo(a, b, 3000.0, MU, 3)


def series_numpy(x):
    """`lambert.hyp2f1b` over an array: (value, terms added, ended by the cap)"""
    res, term, terms, live = np.ones_like(x), np.ones_like(x), np.zeros(x.shape, dtype=int), np.ones(x.shape, dtype=bool)
    for k in range(lambert.SERIES_MAX):
        ii = float(k)
        term = term * ((3.0 + ii) * (1.0 + ii) / (2.5 + ii) * x / (ii + 1.0))
        new = res + term
        terms[live] = k + 1
        live = live & (new != res)
        res = np.where(live | (new == res), new, res)
        if not live.any():
            break
    return res, terms, live


def test_the_series_cap_is_never_binding_and_negative_x_takes_the_closed_form():
    lam = np.linspace(-1.0, 1.0, 803)[1:-1]                         # 801 values inside (-1, 1)
    x = np.linspace(math.sqrt(0.6), math.sqrt(1.4), 403)[1:-1]      # 401 values of x > 0 inside the window
    ll, xx = np.meshgrid(lam, x, indexing="ij")
    assert ((xx > 0.0) & (xx * xx > 0.6) & (xx * xx < 1.4)).all()
    y = np.sqrt(1.0 - (ll * ll) * (1.0 - xx * xx))
    eta = y - ll * xx
    s1 = ((1.0 - ll) - xx * eta) * 0.5
    value, terms, capped = series_numpy(s1)
    print(f"|s1| <= {np.abs(s1).max():.3f}, at most {terms.max()} terms")
    assert np.abs(s1).max() <= 0.4 + 1e-12 and terms.max() <= 43 < lambert.SERIES_MAX and not capped.any()
    for i in range(0, 801, 40):       # the array form above is the scalar definition
        for j in range(0, 401, 40):
            v, t, c = lambert.hyp2f1b(float(s1[i, j]))
            assert (v, t, c) == (value[i, j], terms[i, j], False)
            assert lambert.in_series_window(float(xx[i, j]), 0) and not lambert.in_series_window(float(xx[i, j]), 1)
    # negative x inside 0.6 < x x < 1.4 (solutions live in x > -1): the closed form, finite; the reference's window would have sent
    # the series an argument next to 1, where it needs tens of thousands of terms, and past 1 for an iterate beyond -1
    worst = 0.0
    for lv in (-0.99, -0.5, 0.0, 0.5, 0.99):
        for xv in np.linspace(-0.9999, -math.sqrt(0.6), 23)[:-1]:
            assert not lambert.in_series_window(float(xv), 0) and 0.6 < xv * xv < 1.4
            yv = math.sqrt(1.0 - lv * lv * (1.0 - xv * xv))
            worst = max(worst, ((1.0 - lv) - xv * (yv - lv * xv)) * 0.5)
            assert math.isfinite(lambert.time_of_flight(float(xv), yv, lv, 0))
    assert worst > 0.99 and lambert.hyp2f1b(1.0)[0] == math.inf and lambert.hyp2f1b(0.999)[2]
    # a solved problem whose x lies there, flown to its target
    r1, r2 = np.array([7000.0, 0.0, 0.0]), np.array([0.0, 9000.0, 1000.0])
    hits = 0
    for tof in np.geomspace(2e4, 2e5, 25):
        status, values, _ = lambert.solve(list(r1) + [0.0] * 3, list(r2) + [0.0] * 3, float(tof), MU, Way.ShortWay)
        if status == St.OK and 0.6 < values[P.X] ** 2 < 1.4 and values[P.X] < 0.0:
            hits += 1
            assert flown(r1, r2, float(tof), status, values)[0] < 1e-6
    assert hits >= 3
