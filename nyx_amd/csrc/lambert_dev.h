// lambert_dev.h — what the Lambert kernels (lambert_kernel.hip) evaluate per problem, written so that the SAME TEXT compiles for the
// device and for the host (LMB_FN, as FRM_FN of frame_dev.h).  It restates nyx_amd/lambert.py - the definition, which carries the
// method, its source and the four departures from the reference's izzo.rs (the natural normal, the series window x > 0, the way on
// multi-revolution requests, the closed form of T without its cancellations) - OPERATION FOR OPERATION: one rounding per operation, sums of three as ((a0 + a1) + a2), powers written
// out as products.  Compile with -ffp-contract=off.  The chains go through chain_pv (chain_dev.h), which is included, not copied.
//
// Every loop is bounded on both sides: Halley and Householder by max_iter (<= 1000), the series by NYX_HIP_LMB_SERIES_MAX terms.
#pragma once
#include <math.h>
#include <stdint.h>

#include "frame_dev.h"   // FRM_DEG; chain_dev.h
#include "lambert_args.h"

#define LMB_FN CHAIN_FN
#if defined(__HIPCC__)
#define LMB_OOL static __host__ __device__ __noinline__
#else
#define LMB_OOL static inline
#endif

constexpr double LMB_PI = 3.14159265358979323846;
constexpr double LMB_LN2 = 0.6931471805599453;
constexpr double LMB_TWO_THIRDS = 2.0 / 3.0;
constexpr double LMB_FOUR_THIRDS = 4.0 / 3.0;

struct LmbSol {  // one solved problem: what the sixteen parameters are read from
    double v1[3], v2[3], x, iterations, tof_s, angle_deg, c3, vinf_dep, dla_deg, rla_deg, vinf_arr, dv_total;
};

LMB_FN double lmb_y(double x, double ll) { return sqrt(1.0 - (ll * ll) * (1.0 - x * x)); }

// 2F1(3, 1; 5/2; x) by its series: stops when the sum no longer changes, or at the cap
LMB_FN double lmb_hyp2f1b(double x) {
    if (x >= 1.0) return INFINITY;
    double res = 1.0, term = 1.0, ii = 0.0;
    for (int k = 0; k < NYX_HIP_LMB_SERIES_MAX; ++k) {
        term = term * ((3.0 + ii) * (1.0 + ii) / (2.5 + ii) * x / (ii + 1.0));
        const double old = res;
        res = res + term;
        if (res == old) break;
        ii = ii + 1.0;
    }
    return res;
}

// eta = y - lam x and x - lam y, each by its factored form where lam x > 0 and the difference cancels (the definition says why):
// (y - lam x)(y + lam x) = 1 - lam^2,  (x - lam y)(x + lam y) = (1 - lam^2)(x^2 (1 + lam^2) - lam^2)
LMB_FN double lmb_eta(double x, double y, double ll) {
    if (ll * x > 0.0) return (1.0 - ll * ll) / (y + ll * x);
    return y - ll * x;
}
LMB_FN double lmb_x_minus_lam_y(double x, double y, double ll) {
    if (ll * x > 0.0) {
        const double l2 = ll * ll;
        return ((1.0 - l2) * ((x * x) * (1.0 + l2) - l2)) / (x + ll * y);
    }
    return x - ll * y;
}

// Izzo's auxiliary angle: from sinh psi on a hyperbola, from sin psi AND cos psi on an ellipse (acos alone loses psi next to 0)
LMB_FN double lmb_psi(double x, double y, double ll, double eta) {
    if (x > 1.0) return asinh(eta * sqrt(x * x - 1.0));
    if (x < 1.0) {
        const double om = 1.0 - x * x;
        return atan2(eta * sqrt(om), x * y + ll * om);
    }
    return 0.0;
}

// (out of line on the device: four call sites - the feasibility edge thrice, the Householder loop - share one copy of atan2 / asinh / the series)
// Izzo's non-dimensional time T(x) for m revolutions (`mf` = m as a double): the series next to x = 1 for m == 0, else the closed form
LMB_OOL double lmb_time_of_flight(double x, double y, double ll, double mf) {
    const double xx = x * x;
    const double eta = lmb_eta(x, y, ll);
    if (mf == 0.0 && x > 0.0 && 0.6 < xx && xx < 1.4) {
        const double s1 = ((1.0 - ll) - x * eta) * 0.5;
        const double q = LMB_FOUR_THIRDS * lmb_hyp2f1b(s1);
        return (((eta * eta) * eta) * q + (4.0 * ll) * eta) * 0.5;
    }
    const double psi = lmb_psi(x, y, ll, eta);
    const double den = 1.0 - xx;
    return (((psi + mf * LMB_PI) / sqrt(fabs(den))) - lmb_x_minus_lam_y(x, y, ll)) / den;
}

// T', T'' and T''' at x, from T
LMB_FN void lmb_derivs(double x, double y, double t, double ll, double &d1, double &d2, double &d3) {
    const double l2 = ll * ll, l3 = l2 * ll, l5 = (l2 * l2) * ll;
    const double y2 = y * y, y3 = y2 * y, y5 = (y2 * y2) * y;
    const double om = 1.0 - x * x;
    d1 = (((3.0 * t) * x - 2.0) + ((2.0 * l3) * x) / y) / om;
    d2 = ((3.0 * t + (5.0 * x) * d1) + ((2.0 * (1.0 - l2)) * l3) / y3) / om;
    d3 = (((7.0 * x) * d2 + 8.0 * d1) - (((6.0 * (1.0 - l2)) * l5) * x) / y5) / om;
}

// The minimum of T by Halley's method, T frozen at t0 as the reference writes it: a status, the abscissa in `p`
LMB_FN int lmb_halley(double p0, double t0, double ll, double tol, int max_iter, double &p) {
    for (int it = 0; it < max_iter; ++it) {
        const double y = lmb_y(p0, ll);
        double d1, d2, d3;
        lmb_derivs(p0, y, t0, ll, d1, d2, d3);
        if (fabs(d2) < 1e-14) return NYX_HIP_LMB_TOO_CLOSE;
        p = p0 - ((2.0 * d1) * d2) / (2.0 * (d2 * d2) - d1 * d3);
        if (fabs(p - p0) < tol * fabs(p0) + tol) return NYX_HIP_LMB_OK;
        p0 = p;
    }
    return NYX_HIP_LMB_MAX_ITER_HIT;
}

// The root of T(x) = t0 by Householder's method: a status, the root in `p`, the steps taken in `iters`
LMB_FN int lmb_householder(double p0, double t0, double ll, double mf, double tol, int max_iter, double &p, int &iters) {
    for (int it = 1; it <= max_iter; ++it) {
        const double y = lmb_y(p0, ll);
        const double t = lmb_time_of_flight(p0, y, ll, mf);
        const double fval = t - t0;
        double d1, d2, d3;
        lmb_derivs(p0, y, t, ll, d1, d2, d3);
        const double num = d1 * d1 - (fval * d2) / 2.0;
        const double den = d1 * (d1 * d1 - fval * d2) + (d3 * (fval * fval)) / 6.0;
        if (fabs(den) < 1e-14) return NYX_HIP_LMB_TOO_CLOSE;
        p = p0 - fval * (num / den);
        iters = it;
        if (fabs(p - p0) < tol * fabs(p0) + tol) return NYX_HIP_LMB_OK;
        p0 = p;
    }
    return NYX_HIP_LMB_MAX_ITER_HIT;
}

LMB_FN int lmb_t_min(double ll, double mf, double tol, int max_iter, double &t_min) {
    if (fabs(ll - 1.0) < 1e-9) {
        t_min = lmb_time_of_flight(0.0, lmb_y(0.0, ll), ll, mf);
        return NYX_HIP_LMB_OK;
    }
    const double x_i = 0.1;
    const double t_i = lmb_time_of_flight(x_i, lmb_y(x_i, ll), ll, mf);
    double x_min = x_i;
    if (const int st = lmb_halley(x_i, t_i, ll, tol, max_iter, x_min)) return st;
    t_min = lmb_time_of_flight(x_min, lmb_y(x_min, ll), ll, mf);
    return NYX_HIP_LMB_OK;
}

LMB_FN double lmb_initial_guess(double t, double ll, int m, int high_path) {
    if (m == 0) {
        const double l2 = ll * ll, l3 = l2 * ll, l5 = (l2 * l2) * ll;
        const double t_0 = acos(ll) + ll * sqrt(1.0 - l2);
        const double t_1 = (2.0 * (1.0 - l3)) / 3.0;
        if (t >= t_0) return pow(t_0 / t, LMB_TWO_THIRDS) - 1.0;
        if (t < t_1) return ((((2.5 * t_1) / t) * (t_1 - t)) / (1.0 - l5)) + 1.0;
        return exp((LMB_LN2 * log(t / t_0)) / log(t_1 / t_0)) - 1.0;
    }
    const double mf = (double)m;
    const double term_l = pow((mf * LMB_PI + LMB_PI) / (8.0 * t), LMB_TWO_THIRDS);
    const double x_l = (term_l - 1.0) / (term_l + 1.0);
    const double term_r = pow((8.0 * t) / (mf * LMB_PI), LMB_TWO_THIRDS);
    const double x_r = (term_r - 1.0) / (term_r + 1.0);
    if (high_path) return x_l < x_r ? x_l : x_r;
    return x_l > x_r ? x_l : x_r;
}

LMB_FN double lmb_norm3(double a0, double a1, double a2) { return sqrt((a0 * a0 + a1 * a1) + a2 * a2); }

// One problem: the status; `s` is complete where it is NYX_HIP_LMB_OK.  rv1 / rv2: the bodies' states (the velocities enter C3 .. DV_TOTAL only)
LMB_FN int lmb_solve(const double rv1[6], const double rv2[6], double tof_s, double mu, const nyx_hip_lambert_query_t &q, LmbSol &s) {
    bool finite = __builtin_isfinite(tof_s);
    for (int c = 0; c < 6; ++c) finite = finite && __builtin_isfinite(rv1[c]) && __builtin_isfinite(rv2[c]);
    if (!finite) return NYX_HIP_LMB_BAD_INPUT;
    const double n1 = lmb_norm3(rv1[0], rv1[1], rv1[2]), n2 = lmb_norm3(rv2[0], rv2[1], rv2[2]);
    if (n1 == 0.0 || n2 == 0.0 || !(tof_s > 0.0)) return NYX_HIP_LMB_BAD_INPUT;
    const double c = lmb_norm3(rv2[0] - rv1[0], rv2[1] - rv1[1], rv2[2] - rv1[2]);
    const double sp = ((n1 + n2) + c) * 0.5;
    const double i1[3] = {rv1[0] / n1, rv1[1] / n1, rv1[2] / n1};
    const double i2[3] = {rv2[0] / n2, rv2[1] / n2, rv2[2] / n2};
    const double h0 = i1[1] * i2[2] - i1[2] * i2[1], h1 = i1[2] * i2[0] - i1[0] * i2[2], h2 = i1[0] * i2[1] - i1[1] * i2[0];
    const double hm = lmb_norm3(h0, h1, h2);
    if (c == 0.0 || hm == 0.0) return NYX_HIP_LMB_DEGENERATE;
    const double ih[3] = {h0 / hm, h1 / hm, h2 / hm};
    const double lam = sqrt(1.0 - c / sp);
    bool long_way = q.way == NYX_HIP_LMB_LONG;
    if (q.way == NYX_HIP_LMB_AUTO) {
        double dnu = atan2(rv2[1], rv2[0]) - atan2(rv1[1], rv1[0]);
        if (dnu < 0.0) dnu = dnu + 2.0 * LMB_PI;
        long_way = dnu > LMB_PI;
    }
    const double ll = long_way ? -lam : lam;
    double t1[3], t2[3];
    if (long_way) {   // t_k = i_k x ih
        t1[0] = i1[1] * ih[2] - i1[2] * ih[1]; t1[1] = i1[2] * ih[0] - i1[0] * ih[2]; t1[2] = i1[0] * ih[1] - i1[1] * ih[0];
        t2[0] = i2[1] * ih[2] - i2[2] * ih[1]; t2[1] = i2[2] * ih[0] - i2[0] * ih[2]; t2[2] = i2[0] * ih[1] - i2[1] * ih[0];
    } else {          // t_k = ih x i_k
        t1[0] = ih[1] * i1[2] - ih[2] * i1[1]; t1[1] = ih[2] * i1[0] - ih[0] * i1[2]; t1[2] = ih[0] * i1[1] - ih[1] * i1[0];
        t2[0] = ih[1] * i2[2] - ih[2] * i2[1]; t2[1] = ih[2] * i2[0] - ih[0] * i2[2]; t2[2] = ih[0] * i2[1] - ih[1] * i2[0];
    }
    const double nt1 = lmb_norm3(t1[0], t1[1], t1[2]), nt2 = lmb_norm3(t2[0], t2[1], t2[2]);
    for (int k = 0; k < 3; ++k) { t1[k] = t1[k] / nt1; t2[k] = t2[k] / nt2; }
    const double big_t = sqrt((2.0 * mu) / ((sp * sp) * sp)) * tof_s;
    // find_xy
    const int m = q.n_revs;
    double m_max = floor(big_t / LMB_PI);
    const double t_00 = acos(ll) + ll * sqrt(1.0 - ll * ll);
    if (m_max > 0.0 && big_t < t_00 + m_max * LMB_PI) {
        double t_min = 0.0;
        if (const int st = lmb_t_min(ll, m_max < 2147483648.0 ? m_max : 2147483648.0, q.tol, q.max_iter, t_min)) return st;
        if (big_t < t_min) m_max = m_max - 1.0;
    }
    if ((double)m > m_max) return NYX_HIP_LMB_NOT_FEASIBLE;
    const double x0 = lmb_initial_guess(big_t, ll, m, q.high_path);
    double x = x0;
    int iters = 0;
    if (const int st = lmb_householder(x0, big_t, ll, (double)m, q.tol, q.max_iter, x, iters)) return st;
    // reconstruct
    const double y = lmb_y(x, ll);
    const double gamma = sqrt((mu * sp) / 2.0);
    const double rho = (n1 - n2) / c;
    const double sigma = sqrt(1.0 - rho * rho);
    const double a = ll * y - x, b = ll * y + x;
    const double v_r1 = (gamma * (a - rho * b)) / n1;
    const double v_r2 = ((-gamma) * (a + rho * b)) / n2;
    const double v_t1 = ((gamma * sigma) * (y + ll * x)) / n1;
    const double v_t2 = ((gamma * sigma) * (y + ll * x)) / n2;
    for (int k = 0; k < 3; ++k) {
        s.v1[k] = v_r1 * i1[k] + v_t1 * t1[k];
        s.v2[k] = v_r2 * i2[k] + v_t2 * t2[k];
    }
    s.x = x;
    s.iterations = (double)iters;
    s.tof_s = tof_s;
    const double cosd = (i1[0] * i2[0] + i1[1] * i2[1]) + i1[2] * i2[2];
    double ang = acos(cosd < -1.0 ? -1.0 : (cosd > 1.0 ? 1.0 : cosd)) * FRM_DEG;
    if (long_way) ang = 360.0 - ang;
    s.angle_deg = ang + 360.0 * (double)m;
    const double w0 = s.v1[0] - rv1[3], w1 = s.v1[1] - rv1[4], w2 = s.v1[2] - rv1[5];
    s.c3 = (w0 * w0 + w1 * w1) + w2 * w2;
    s.vinf_dep = sqrt(s.c3);
    s.vinf_arr = lmb_norm3(rv2[3] - s.v2[0], rv2[4] - s.v2[1], rv2[5] - s.v2[2]);
    s.dla_deg = asin(w2 / s.vinf_dep) * FRM_DEG;
    s.rla_deg = atan2(w1, w0) * FRM_DEG;
    s.dv_total = s.vinf_dep + s.vinf_arr;
    return NYX_HIP_LMB_OK;
}

// `param` is the same for every lane (a kernel argument): a scalar branch
LMB_FN double lmb_param(int32_t param, const LmbSol &s) {
    switch (param) {
    case NYX_HIP_LMB_V1X: return s.v1[0];
    case NYX_HIP_LMB_V1Y: return s.v1[1];
    case NYX_HIP_LMB_V1Z: return s.v1[2];
    case NYX_HIP_LMB_V2X: return s.v2[0];
    case NYX_HIP_LMB_V2Y: return s.v2[1];
    case NYX_HIP_LMB_V2Z: return s.v2[2];
    case NYX_HIP_LMB_X: return s.x;
    case NYX_HIP_LMB_ITERATIONS: return s.iterations;
    case NYX_HIP_LMB_TOF_S: return s.tof_s;
    case NYX_HIP_LMB_TRANSFER_ANGLE_DEG: return s.angle_deg;
    case NYX_HIP_LMB_C3: return s.c3;
    case NYX_HIP_LMB_VINF_DEP: return s.vinf_dep;
    case NYX_HIP_LMB_DLA_DEG: return s.dla_deg;
    case NYX_HIP_LMB_RLA_DEG: return s.rla_deg;
    case NYX_HIP_LMB_VINF_ARR: return s.vinf_arr;
    case NYX_HIP_LMB_DV_TOTAL: return s.dv_total;
    default: return __builtin_nan("");
    }
}

// A body's state about the centre at et_s: chain(body) - chain(centre), component by component
LMB_FN int lmb_body_state(const ResolvedChain &body, const ResolvedChain &centre, const double *records, double et_s, double rv6[6]) {
    double b[6], c[6];
    const int st_b = chain_pv(body, records, et_s, b);
    const int st_c = chain_pv(centre, records, et_s, c);
    for (int k = 0; k < 6; ++k) rv6[k] = b[k] - c[k];
    return st_b ? st_b : st_c;
}
