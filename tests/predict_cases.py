"""Shared inputs and references of the covariance-mapping tests (nyx_hip_predict_until against nyx_oracle_predict_until):
the batches, epochs and process-noise lists that the CPU tests (test_predict_cases.py) and the device tests
(test_gpu_predict.py, test_gpu_predict_loop.py) both run, an extended-precision recomputation of the Kalman time update,
and a threaded front of the serial oracle."""
import dataclasses
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import nyx_amd as nx
import oracle_lib
from nyx_amd import _abi, ephem, od
from scenarios import EPOCH0_NS, dispersed_leo_batch, keplerian_to_cartesian, leo_full_setup

S = nx.NS_PER_S


def geo_batch(n, seed):
    b = dispersed_leo_batch(n, seed=seed)
    geo = keplerian_to_cartesian(42164.0, 1e-5, 0.0, 163.0, 75.0, 0.0, ephem.MU_EARTH)   # examples/03_geo_analysis/drift.rs:50
    rv = b.rv()
    b.set_rv(geo[None, :] + (rv - rv.mean(axis=0)))
    return b


def init_covar(n, seed=0):
    rng = np.random.default_rng(seed)
    out = np.zeros((n, 9, 9))
    for i in range(n):
        a = rng.standard_normal((9, 9)) * np.array([1.0, 1.0, 1.0, 1e-3, 1e-3, 1e-3, 1e-2, 0.0, 0.0])[:, None]
        out[i] = a @ a.T
    return out


def rel_err(got, ref):
    scale = np.maximum(np.abs(ref), 1e-6 * np.abs(ref).max(axis=(-2, -1), keepdims=True))
    return (np.abs(got - ref) / scale).max()


def dev_err(got, ref):
    """Deviation vectors: the largest element error over the largest reference element (as test_gpu_predict.py does)."""
    return np.abs(got - ref).max() / np.abs(ref).max()


def coverage_end_ns(almanac):
    """The last epoch every ephemeris segment of `almanac` covers (the earliest init_et_s + interval_s * n_records), in the
    nanoseconds of the batch epochs.  Subtract EPOCH0_NS for the offset to the scenarios' epoch."""
    end_s = min(seg.init_et_s + seg.interval_s * seg.records.shape[0] for seg in almanac.segments)
    whole = int(np.floor(end_s))                       # (seconds past J2000 times 1e9 does not fit a double's mantissa)
    return whole * S + int(round((end_s - whole) * 1e9))


# ---------------------------------------------------------------------------------------------
# KalmanFilter::time_update (od/kalman/filtering.rs:59-99) with ProcessNoise::to_matrix / ::propagate (od/snc.rs:165-283),
# recomputed from their definitions in extended precision
# ---------------------------------------------------------------------------------------------

class _LongDouble:
    """x87 extended precision (63-bit mantissa) where numpy's longdouble is one."""
    name = "longdouble"

    @staticmethod
    def num(x):
        return np.longdouble(x)

    @staticmethod
    def ratio(a, b):
        return np.longdouble(int(a)) / np.longdouble(int(b))

    sqrt = staticmethod(np.sqrt)
    exp = staticmethod(np.exp)


class _Mp:
    """mpmath at 50 digits, where the platform's longdouble is a plain double."""
    name = "mpmath"

    @staticmethod
    def num(x):
        import mpmath
        return mpmath.mpf(float(x))

    @staticmethod
    def ratio(a, b):
        import mpmath
        return mpmath.mpf(int(a)) / mpmath.mpf(int(b))

    @staticmethod
    def sqrt(x):
        import mpmath
        return mpmath.sqrt(x)

    @staticmethod
    def exp(x):
        import mpmath
        return mpmath.exp(x)


def _backend(force_mpmath=False):
    if not force_mpmath and np.finfo(np.longdouble).nmant > 52:
        return _LongDouble
    import mpmath
    mpmath.mp.dps = 50
    return _Mp


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _unit(xp, a):
    n = xp.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])
    return [a[0] / n, a[1] / n, a[2] / n]


def _matmul(a, b, rows, inner, cols):
    return [[sum((a[r][k] * b[k][c] for k in range(1, inner)), a[r][0] * b[0][c]) for c in range(cols)] for r in range(rows)]


def snc_diagonal(xp, pn, epoch_ns, init_epoch_ns, nominal):
    """ProcessNoise::to_matrix's diagonal at `epoch_ns` (constant, or decayed since the initial estimate's epoch), expressed in the
    state frame as ProcessNoise::propagate does: dcm * snc * dcm^T at the nominal orbit, the diagonal kept."""
    d = [xp.num(v) for v in pn.diag]
    if pn.decay_s is not None:
        init = init_epoch_ns if pn.init_epoch_ns is None else pn.init_epoch_ns
        total = xp.ratio(int(epoch_ns) - int(init), S)
        d = [d[k] * xp.exp(-xp.num(pn.decay_s[k]) * total) for k in range(3)]
    if pn.local_frame is not None:
        r, v = [xp.num(x) for x in nominal[:3]], [xp.num(x) for x in nominal[3:6]]
        c_hat = _unit(xp, _cross(r, v))                                # orbit normal
        if pn.local_frame == "RIC":
            r_hat = _unit(xp, r)
            cols = [r_hat, _cross(c_hat, r_hat), c_hat]
        elif pn.local_frame == "VNC":
            v_hat = _unit(xp, v)
            cols = [v_hat, c_hat, _cross(v_hat, c_hat)]
        else:
            raise NotImplementedError(pn.local_frame)
        d = [sum(cols[j][k] * d[j] * cols[j][k] for j in range(3)) for k in range(3)]
    return d


def select_noise(process_noise, epoch_ns, delta_ns):
    """filtering.rs:64-80: the entries are tried last first; one that has not started (snc.rs:168-175) or whose disable time the
    update's span exceeds (snc.rs:178-186, 257-259) is passed over.  Index of the entry that applies, or None."""
    for q in range(len(process_noise) - 1, -1, -1):
        pn = process_noise[q]
        if pn.start_time_ns is not None and pn.start_time_ns > epoch_ns:
            continue
        if delta_ns > pn.disable_time_ns:
            continue
        return q
    return None


def time_update_reference(p0, stm_hist, epochs_ns, nominal_hist, n_updates, epoch0_ns, process_noise, max_hist, dev0=None,
                          force_mpmath=False):
    """P-bar = Phi P Phi^T + Gamma Q Gamma^T and dev = Phi dev of ONE run, update after update from `p0` (and `dev0`), with the given
    Phi, epoch and nominal-state history ([updates, ...] of that run) in extended precision (numpy's longdouble where it has more than
    52 mantissa bits, mpmath at 50 digits otherwise); the intermediate covariances are not rounded to double.
    -> (covar[m, 9, 9], dev[m, 9], noise[m, 9, 9]) as doubles, m = min(n_updates, max_hist); noise = the Gamma Q Gamma^T that was added."""
    xp = _backend(force_mpmath)
    m = min(int(n_updates), int(max_hist))
    p = [[xp.num(p0[r][c]) for c in range(9)] for r in range(9)]
    dev = [[xp.num(0.0 if dev0 is None else dev0[r])] for r in range(9)]
    covar, devs, noise = np.zeros((m, 9, 9)), np.zeros((m, 9)), np.zeros((m, 9, 9))
    prev = int(epoch0_ns)
    for u in range(m):
        phi = [[xp.num(stm_hist[u][r][c]) for c in range(9)] for r in range(9)]
        phi_t = [[phi[c][r] for c in range(9)] for r in range(9)]
        p = _matmul(_matmul(phi, p, 9, 9, 9), phi_t, 9, 9, 9)
        dev = _matmul(phi, dev, 9, 9, 1)
        epoch = int(epochs_ns[u])
        delta = epoch - prev
        q = select_noise(process_noise, epoch, delta)
        if q is not None:
            d = snc_diagonal(xp, process_noise[q], epoch, int(epoch0_ns), nominal_hist[u])
            dt = xp.ratio(delta, S)
            gamma = [dt * dt / xp.num(2.0)] * 3 + [dt] * 3           # rows 0-2: dt^2 / 2, rows 3-5: dt, onto column row % 3
            for r in range(6):
                for c in range(6):
                    if r % 3 == c % 3:
                        add = gamma[r] * d[r % 3] * gamma[c]
                        p[r][c] = p[r][c] + add
                        noise[u, r, c] = float(add)
        covar[u] = [[float(x) for x in row] for row in p]
        devs[u] = [float(row[0]) for row in dev]
        prev = epoch
    return covar, devs, noise


def reference_errors(res, p0, epoch0_ns, process_noise, dev0=None, runs=None):
    """(worst rel_err of covar_history, worst dev_err of deviation_history) of a Predicted against time_update_reference fed the
    result's OWN Phi, epoch and nominal history, over `runs` (default: every run with an update)."""
    cap = res.covar_history.shape[0]
    e_p = e_d = 0.0
    for i in (range(len(res.n_updates)) if runs is None else runs):
        if res.n_updates[i] == 0:
            continue
        covar, devs, _ = time_update_reference(p0[i], res.stm[:, i], res.epochs_ns[:, i], res.nominal[:, i], res.n_updates[i], epoch0_ns[i],
                                               process_noise, cap, None if dev0 is None else dev0[i])
        m = covar.shape[0]
        e_p = max(e_p, rel_err(res.covar_history[:m, i], covar))
        if dev0 is not None:
            e_d = max(e_d, dev_err(res.deviation_history[:m, i], devs))
    return e_p, e_d


# ---------------------------------------------------------------------------------------------
# the serial oracle over a thread pool (ctypes releases the interpreter lock; nyx_oracle_predict_until keeps no state)
# ---------------------------------------------------------------------------------------------

def oracle_predict_threaded(compiled, batch, p0, end_epoch_ns, max_step_ns, n_threads=16, **kw):
    """oracle_lib.predict_until on the slices k::n_threads of the batch, one per thread, put back in the batch's order."""
    n = batch.n
    p0 = np.asarray(p0, dtype=np.float64).reshape(n, 9, 9)
    dev0 = kw.pop("state_deviation", None)
    parts = [np.arange(k, n, n_threads) for k in range(min(n_threads, n))]

    def run(idx):
        extra = {} if dev0 is None else {"state_deviation": np.asarray(dev0, dtype=np.float64).reshape(n, 9)[idx]}
        return oracle_lib.predict_until(compiled, batch.take(idx), p0[idx], end_epoch_ns, max_step_ns, **extra, **kw)

    with ThreadPoolExecutor(max_workers=len(parts)) as pool:
        results = list(pool.map(run, parts))
    out, stats = batch.copy(), _abi.StatsBatch(n)
    out.stm = np.zeros((n, 81))
    res = od.Predicted(out, stats, np.zeros((n, 9, 9)), np.zeros((n, 9)), np.zeros(n, dtype=np.int32))
    first = results[0]
    for f in ("epochs_ns", "nominal", "stm", "covar_history", "deviation_history"):
        v = getattr(first, f)
        if v is not None:
            setattr(res, f, np.zeros((v.shape[0], n) + v.shape[2:], dtype=v.dtype))
    for idx, r in zip(parts, results):
        for f in ["epoch_ns", "stm", "step_ns"] + _abi.F64_FIELDS:
            getattr(out, f)[idx] = getattr(r.states, f)
        for f in ("status", "last_step_ns", "last_error", "last_attempts", "n_accepted", "n_rejected", "n_evals"):
            getattr(stats, f)[idx] = getattr(r.stats, f)
        res.covar[idx], res.state_deviation[idx], res.n_updates[idx] = r.covar, r.state_deviation, r.n_updates
        for f in ("epochs_ns", "nominal", "stm", "covar_history", "deviation_history"):
            if getattr(res, f) is not None:
                getattr(res, f)[:, idx] = getattr(r, f)
    return res


# ---------------------------------------------------------------------------------------------
# the cases: dict(prop, almanac, central) of a force model, and dict(batch, p0, dev0, end, max_step, noise, history) of a run
# ---------------------------------------------------------------------------------------------

def loop_noise(frame="RIC"):
    """Decaying process noise defined in a local frame: every branch of the noise arithmetic at each update."""
    return [nx.ProcessNoise3D.with_decay([1e-12, 2e-12, 3e-12], 3600 * S, [1e-4, 2e-4, 0.0], local_frame=frame)]


def _case(batch, end, max_step, history, noise, covar_seed=2):
    n = batch.n
    batch.stm = np.zeros((n, 81)); batch.reset_stm()
    return dict(batch=batch, p0=init_covar(n, covar_seed), dev0=np.random.default_rng(3).standard_normal((n, 9)) * 1e-3,
                end=end, max_step=max_step, history=history, noise=noise)


def kwargs(case, keep_stm=True):
    """The keyword arguments of predict_until (device or oracle) for a case: noise, deviation tracking, history."""
    return dict(process_noise=case["noise"], deviation_tracking=True, state_deviation=case["dev0"], history=case["history"], keep_stm=keep_stm)


def shapes_case(n):
    """GEO, 60 s segments (single RK89 attempts), ragged starts: 5 or 6 updates to the common end, more than the history keeps."""
    b = geo_batch(n, 13)
    b.epoch_ns[:] = EPOCH0_NS + (np.arange(n) % 4) * 45 * S
    return _case(b, EPOCH0_NS + 360 * S, 60 * S, 4, loop_noise())


SHAPE_SIZES = (1, 16, 17, 33)       # one trajectory; a full workgroup of the sixteen-per-workgroup layout; one more; two and one more


def adaptive_case(n=33):
    """LEO, RK89 with its default options, 600 s segments of about ten accepted steps with rejections, ragged starts."""
    b = dispersed_leo_batch(n, seed=21)
    b.epoch_ns[:] = EPOCH0_NS + (np.arange(n) % 4) * 200 * S
    return _case(b, EPOCH0_NS + 3600 * S, 600 * S, 6, loop_noise())


def fixed_step_setup(degree):
    return leo_full_setup(degree=degree, method=nx.IntegratorMethod.RungeKutta4, opts=nx.IntegratorOptions.with_fixed_step_s(10.0))


def fixed_case(n=33):
    """LEO, RK4 at a fixed 10 s, 30 s segments of three steps, ragged starts: 4 or 5 updates."""
    b = dispersed_leo_batch(n, seed=22)
    b.epoch_ns[:] = EPOCH0_NS + (np.arange(n) % 4) * 10 * S
    return _case(b, EPOCH0_NS + 150 * S, 30 * S, 5, loop_noise())


FAILURE_OFFSETS_S = (480, 130, 360, 250, 240, 10, 120, 370)     # start = end - offset; 120 s segments of twelve fixed 10 s RK4 steps
FAILURE_END_BEFORE_COVERAGE_S = 52                              # stage epochs (c = 0, 1/2, 1/2, 1) fall at -2, +3, +3, +8 s of the coverage end
FAILURE_STEP_S, FAILURE_SEGMENT_S = 10, 120


def failure_case(almanac, n):
    """Runs that leave the almanac's coverage in a LATER segment than their first, next to runs that end just inside it: a run whose
    offset is a multiple of 120 s lands on `end` and stops; the others go on for one more segment and meet the coverage end in it."""
    end = coverage_end_ns(almanac) - FAILURE_END_BEFORE_COVERAGE_S * S
    b = dispersed_leo_batch(n, seed=23)
    b.epoch_ns[:] = end - np.resize(np.array(FAILURE_OFFSETS_S), n) * S
    return _case(b, end, FAILURE_SEGMENT_S * S, 4, loop_noise())


def failure_stage_epochs(case):
    """Every RK4 stage epoch [run][...] (ns) the runs of failure_case would evaluate if nothing failed, up to their last segment."""
    out = []
    for e0 in case["batch"].epoch_ns:
        n_seg = max(1, -(-(case["end"] - int(e0)) // case["max_step"]))
        starts = int(e0) + np.arange(n_seg * (FAILURE_SEGMENT_S // FAILURE_STEP_S)) * FAILURE_STEP_S * S
        out.append(np.concatenate([starts, starts + FAILURE_STEP_S * S // 2, starts + FAILURE_STEP_S * S]))
    return out


def selection_case(kind, n=17):
    """The process-noise selections of filtering.rs:64-80 that need more than one entry or more than one update to show, GEO, four 60 s
    updates.  -> (case, twin): `twin` is the noise list whose run the case must reproduce bit for bit, over the updates `twin_updates`.
    'disable': the last entry's disable time (30 s) is shorter than the 60 s updates, so the first entry applies at every update;
    'late': one entry that starts 150 s in: the updates at 60 and 120 s carry no noise, those at 180 and 240 s do;
    'init_epoch': a decaying entry whose decay clock starts 100 s before the batch's epoch (ProcessNoise::init_epoch)."""
    b = geo_batch(n, 14)
    if kind == "disable":
        first = nx.ProcessNoise3D.from_diagonal([1e-11] * 3, 10 * 60 * S)
        noise, twin, twin_updates = [first, nx.ProcessNoise3D.from_diagonal([5e-11] * 3, 30 * S)], [first], slice(0, 4)
    elif kind == "late":
        noise, twin, twin_updates = [nx.ProcessNoise3D.with_start_time(10 * 60 * S, [1e-11] * 3, EPOCH0_NS + 150 * S)], [], slice(0, 2)
    elif kind == "init_epoch":
        pn = nx.ProcessNoise3D.with_decay([1e-11, 4e-11, 9e-11], 10 * 60 * S, [5e-3, 1e-2, 0.0])
        noise, twin, twin_updates = [dataclasses.replace(pn, init_epoch_ns=EPOCH0_NS - 100 * S)], None, slice(0, 0)
    else:
        raise ValueError(kind)
    case = _case(b, EPOCH0_NS + 240 * S, 60 * S, 4, noise)
    case["twin"], case["twin_updates"] = twin, twin_updates
    return case


REFERENCE_DIAG, REFERENCE_DECAY = [1e-11, 4e-11, 9e-11], [5e-3, 1e-2, 0.0]


def reference_case(frame, n=40):
    """The runs time_update_reference itself is checked on against the oracle: LEO, six 60 s updates, decaying noise in `frame`, half of
    the runs starting 17 s later (each run has its own decay clock)."""
    b = dispersed_leo_batch(n, seed=9)
    b.epoch_ns[: n // 2] += 17 * S
    noise = [nx.ProcessNoise3D.with_decay(REFERENCE_DIAG, 10 * 60 * S, REFERENCE_DECAY, local_frame=frame)]
    return _case(b, EPOCH0_NS + 6 * 60 * S, 60 * S, 6, noise)
