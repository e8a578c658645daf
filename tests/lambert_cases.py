"""What tests/test_gpu_lambert.py and tests/test_lambert_host_cxx.py share: the seeded batch of problems and the bounds of a comparison
with the host definition (nyx_amd/lambert.py), derived in the docstring of tests/test_gpu_lambert.py."""
import math

import numpy as np

from nyx_amd.lambert import LambertParameter as P

EPS = 2.0 ** -52
K = 18.0
MARGIN = 1e-6
MU_EARTH = 398600.435436096
VEC = {P.V1X: 0, P.V1Y: 0, P.V1Z: 0, P.V2X: 1, P.V2Y: 1, P.V2Z: 1}


def bounds(want, extras, rv1, rv2):
    """The bound of every parameter for every problem: want [16, N], extras [N], rv1 / rv2 [6, N] -> [16, N] (NaN where not solved)."""
    n = want.shape[1]
    out = np.full((len(P), n), np.nan)
    for i in range(n):
        ex = extras[i]
        if "dT_dx" not in ex:
            continue
        v = want[:, i]
        lever = abs(ex["T"] / ex["dT_dx"])
        dv = [K * EPS * (lever * np.linalg.norm(ex["dv_dx"][3 * k:3 * k + 3]) + np.linalg.norm(v[3 * k:3 * k + 3])) for k in (0, 1)]
        for p, k in VEC.items():
            out[p, i] = dv[k]
        out[P.X, i] = K * EPS * (lever + abs(v[P.X]))
        out[P.Iterations, i] = out[P.TofS, i] = 0.0
        out[P.TransferAngleDeg, i] = 1e-12
        w = v[0:3] - rv1[3:6, i]
        wn, wxy = np.linalg.norm(w), math.hypot(w[0], w[1])
        out[P.C3, i] = 2.0 * wn * dv[0] + 4.0 * EPS * v[P.C3]
        out[P.VinfDep, i] = dv[0] + 2.0 * EPS * wn
        out[P.VinfArr, i] = dv[1] + 2.0 * EPS * v[P.VinfArr]
        out[P.DvTotal, i] = out[P.VinfDep, i] + out[P.VinfArr, i] + EPS * v[P.DvTotal]
        out[P.RlaDeg, i] = math.degrees(dv[0] / wxy) + 1e-12
        out[P.DlaDeg, i] = math.degrees(dv[0] / wn + 8.0 * EPS / math.cos(math.radians(v[P.DlaDeg]))) + 1e-12
    return out


def problems(seed=1, n=70):
    """60 seeded problems about the Earth, (r1 x r2).z < 0 in every other one, and ten hand-made ones: rv1 [6, n], rv2 [6, n], tof_s [n]."""
    rng = np.random.default_rng(seed)
    m = n - 10
    d1, d2 = rng.normal(size=(m, 3)), rng.normal(size=(m, 3))
    r1 = d1 / np.linalg.norm(d1, axis=1)[:, None] * rng.uniform(7000.0, 42000.0, size=(m, 1))
    r2 = d2 / np.linalg.norm(d2, axis=1)[:, None] * rng.uniform(7000.0, 42000.0, size=(m, 1))
    mirror = ((np.arange(m) % 2 == 0) != (np.cross(r1, r2)[:, 2] < 0.0))[:, None] * np.array([0.0, -2.0, 0.0]) + 1.0
    r1, r2 = r1 * mirror, r2 * mirror
    rv1 = np.concatenate([r1, rng.normal(size=(m, 3)) * 3.0], axis=1)
    rv2 = np.concatenate([r2, rng.normal(size=(m, 3)) * 3.0], axis=1)
    tof = 10.0 ** rng.uniform(3.3, 5.5, size=m)
    a, b = [7000.0, 0.0, 0.0, 0.0, 7.5, 0.0], [6000.0, 3000.0, 500.0, -3.0, 6.0, 1.0]
    special = [([math.nan] + a[1:], b, 3000.0), ([0.0, 0.0, 0.0, 0.0, 7.5, 0.0], b, 3000.0), (a, b, 0.0), (a, b, -5.0), (a, b[:5] + [math.inf], 3000.0),   # BAD_INPUT
               (a, a, 3000.0), (a, [14000.0, 0.0, 0.0, 0.0, 5.0, 0.0], 3000.0), (a, [-7000.0, 0.0, 0.0, 0.0, -7.5, 0.0], 3000.0),                     # DEGENERATE
               (a, b, 1e-3),                                                                                                                        # TOO_CLOSE
               ([15945.34, 0.0, 0.0, 0.0, 0.0, 0.0], [12214.83899, 10249.46731, 0.0, 0.0, 0.0, 0.0], 4560.0)]                                       # Vallado 7-1
    rv1 = np.concatenate([rv1, np.array([s[0] for s in special])]).T.copy()
    rv2 = np.concatenate([rv2, np.array([s[1] for s in special])]).T.copy()
    return rv1, rv2, np.concatenate([tof, [s[2] for s in special]])
