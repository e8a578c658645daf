// target_dev.h — what the targeter kernels (target_kernel.hip) do per run, written so that the SAME TEXT compiles for the device and
// for the host (TGT_FN): tests/cxx/target_host_check.cpp runs the very code of the kernels on the CPU.  It restates
// nyx_amd/targeter.py (`target_definition`) operation for operation; include/nyx_hip_target.h states the definition.
//   tgt_c6 / tgt_apply     a correction of the variables as a 6-vector, applied in the inertial frame or in the VNC frame of a state
//   tgt_seed               xi and total of a run from xi_start and the initial guesses
//   tgt_start_state        start state k of a round: k = 0 the nominal xi, k = 1 .. V the perturbed states
//   tgt_step               one round of a run from its 1 + V final states: the objectives (frm_value's pieces, frame_dev.h), the error,
//                          the tests, the Jacobian, the Cholesky solve, the clamp and the update of xi and total
//   tgt_corrected          xi_start with the total applied
// O <= 6 objectives and V <= 6 variables.  Every loop over them runs over the compile-time maximum with a guard, and the one loop
// that is rolled (over the 1 + V final states) writes its column of the Jacobian through a chain of selects: no register array is
// indexed at run time, nothing goes to scratch.  The sizes and codes are the same for every lane (kernel arguments).
// Compile with -ffp-contract=off: one rounding per operation.
#pragma once
#include <math.h>
#include <stdint.h>

#include "frame_dev.h"
#include "target_args.h"

#if defined(__HIPCC__)
#define TGT_FN static __host__ __device__ __forceinline__
#define TGT_UNROLL _Pragma("unroll")
#define TGT_ROLLED _Pragma("unroll 1")
#else
#define TGT_FN static inline
#define TGT_UNROLL
#define TGT_ROLLED
#endif

constexpr int TGT_MV = NYX_HIP_MAX_TARGET_VARS, TGT_MO = NYX_HIP_MAX_TARGET_OBJS;
constexpr int TGT_GOES_ON = -1;   // tgt_step: the run takes another round

// What a run carries from round to round
struct TgtRun {
    double xi[6];          // the nominal state at the correction epoch, corrections applied
    double total[TGT_MV];  // the sum of the corrections, per variable
    double prev;           // |err| of the round before; +inf before the first
};

TGT_FN bool tgt_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }   // (false for a NaN)

// c6 = 0, then c6[component_j] = c6[component_j] + val[j] in the order of the variables
TGT_FN void tgt_c6(const nyx_hip_target_query_t &q, const double val[TGT_MV], double c6[6]) {
TGT_UNROLL
    for (int k = 0; k < 6; ++k) c6[k] = 0.0;
TGT_UNROLL
    for (int j = 0; j < TGT_MV; ++j)
        if (j < q.n_vars) {
TGT_UNROLL
            for (int k = 0; k < 6; ++k)
                if (q.var_component[j] == k) c6[k] = c6[k] + val[j];
        }
}

// x = x (+) c6.  Inertial: component by component.  VNC: the velocity takes [e0, e1, e2] c6[3..6] with e0 = v^, e1 = (r x v)^,
// e2 = e0 x e1 of `from` (the frame predict_kernel.hip forms for its process noise); the position stays (no position variable there).
// Every caller passes xi_start as `from`: one frame per run, so that the total of the steps, applied once, is the state they led to
TGT_FN void tgt_apply(int32_t frame, const double from[6], const double c6[6], double x[6]) {
    if (frame == NYX_HIP_FRAME_VNC) {
        const double h0 = from[1] * from[5] - from[2] * from[4], h1 = from[2] * from[3] - from[0] * from[5], h2 = from[0] * from[4] - from[1] * from[3];
        const double hn = sqrt((h0 * h0 + h1 * h1) + h2 * h2);
        const double vn = sqrt((from[3] * from[3] + from[4] * from[4]) + from[5] * from[5]);
        const double e00 = from[3] / vn, e01 = from[4] / vn, e02 = from[5] / vn;
        const double e10 = h0 / hn, e11 = h1 / hn, e12 = h2 / hn;
        const double e20 = e01 * e12 - e02 * e11, e21 = e02 * e10 - e00 * e12, e22 = e00 * e11 - e01 * e10;
        x[3] = x[3] + ((e00 * c6[3] + e10 * c6[4]) + e20 * c6[5]);
        x[4] = x[4] + ((e01 * c6[3] + e11 * c6[4]) + e21 * c6[5]);
        x[5] = x[5] + ((e02 * c6[3] + e12 * c6[4]) + e22 * c6[5]);
    } else {
TGT_UNROLL
        for (int k = 0; k < 6; ++k) x[k] = x[k] + c6[k];
    }
}

TGT_FN void tgt_seed(const nyx_hip_target_query_t &q, const double xi_start[6], TgtRun &run) {
    double c6[6], from[6];
    tgt_c6(q, q.var_init_guess, c6);
TGT_UNROLL
    for (int k = 0; k < 6; ++k) run.xi[k] = from[k] = xi_start[k];
    tgt_apply(q.correction_frame, from, c6, run.xi);
TGT_UNROLL
    for (int j = 0; j < TGT_MV; ++j) run.total[j] = j < q.n_vars ? q.var_init_guess[j] : 0.0;
    run.prev = (double)INFINITY;
}

// start state k of a round (k is the same for every lane); `frm` is xi_start: its VNC frame is THE correction frame of the run
TGT_FN void tgt_start_state(const nyx_hip_target_query_t &q, const double frm[6], const double xi[6], int k, double x[6]) {
TGT_UNROLL
    for (int c = 0; c < 6; ++c) x[c] = xi[c];
    if (k == 0) return;
    double only[6];   // c6 of the one variable of this state: 0 + perturbation_j at its component
TGT_UNROLL
    for (int c = 0; c < 6; ++c) only[c] = 0.0;
TGT_UNROLL
    for (int j = 0; j < TGT_MV; ++j)
        if (j == k - 1) {
TGT_UNROLL
            for (int c = 0; c < 6; ++c)
                if (q.var_component[j] == c) only[c] = only[c] + q.var_perturbation[j];
        }
    tgt_apply(q.correction_frame, frm, only, x);
}

TGT_FN void tgt_corrected(const nyx_hip_target_query_t &q, const double xi_start[6], const double total[TGT_MV], double x[6]) {
    double c6[6];
    tgt_c6(q, total, c6);
TGT_UNROLL
    for (int k = 0; k < 6; ++k) x[k] = xi_start[k];
    tgt_apply(q.correction_frame, xi_start, c6, x);
}

// One round of one run.  `load(k, y)` delivers the final state of row k ABOUT THE OBJECTIVE TARGET and returns the row's propagation
// status; `need`: tgt_needs(q), worked out on the host; `ephem_bad`: the target's state does not exist at the achievement epoch.
// `park` / `ps`: 36 doubles of the run's own, element e at park[e * ps] - the Jacobian is written there entry by entry while the
// parameters are evaluated (an index that is not known at compile time is an address, not a register) and read back for the solve, so
// that it is not held in registers beside the parameter code.  `frm_at` / `fs`: xi_start (the correction frame), component k at frm_at[k * fs].  Returns a nyx_hip_target_status when the run ends in this round,
// TGT_GOES_ON when run.xi / run.total / run.prev hold the next round's.  err[i] (i < n_objs) is written unless the run ends with
// EPHEM_RANGE or PROP_FAILED, where it is NaN.
template <typename Load>
TGT_FN int tgt_step(const nyx_hip_target_query_t &q, int32_t need, int it, bool ephem_bad, Load load, double *park, int64_t ps, const double *frm_at,
                    int64_t fs, TgtRun &run, double err[TGT_MO]) {
    const int V = q.n_vars, O = q.n_objs;
    double val0[TGT_MO];
TGT_UNROLL
    for (int i = 0; i < TGT_MO; ++i) {
        val0[i] = 0.0;
        err[i] = __builtin_nan("");
    }
    bool prop_bad = false, not_finite = false;
TGT_ROLLED
    for (int k = 0; k <= V; ++k) {
        double y[6];
        prop_bad = (load(k, y) != NYX_HIP_OK) || prop_bad;
        FrmShared s = {};   // (only what `need` names is formed)
        frm_shared(need, q.mu_km3_s2, y, s);
        double pert = 1.0;   // perturbation_{k - 1}
TGT_UNROLL
        for (int j = 0; j < TGT_MV; ++j)
            if (j == k - 1) pert = q.var_perturbation[j];
TGT_ROLLED   // (one copy of the parameter code; i and obj_param[i] are the same for every lane)
        for (int i = 0; i < O; ++i) {
            const double v = frm_param(q.obj_param[i], q.mu_km3_s2, y, s);
            if (k == 0) {
                not_finite = !tgt_finite(v) || not_finite;
TGT_UNROLL
                for (int ii = 0; ii < TGT_MO; ++ii) val0[ii] = ii == i ? v : val0[ii];
            } else {
                double v0 = 0.0;   // val0[i]
TGT_UNROLL
                for (int ii = 0; ii < TGT_MO; ++ii) v0 = ii == i ? val0[ii] : v0;
                const double d = (v - v0) / pert;
                not_finite = !tgt_finite(d) || not_finite;
                park[(int64_t)(i * TGT_MV + (k - 1)) * ps] = d;
            }
        }
    }
    if (ephem_bad) return NYX_HIP_TGT_EPHEM_RANGE;
    if (prop_bad) return NYX_HIP_TGT_PROP_FAILED;
    bool conv = true;
TGT_UNROLL
    for (int i = 0; i < TGT_MO; ++i)
        if (i < O) {
            err[i] = q.obj_mult[i] * (q.obj_desired[i] - val0[i]) + q.obj_add[i];
            conv = conv && fabs(err[i]) <= q.obj_tolerance[i];
        }
    if (not_finite) return NYX_HIP_TGT_NOT_FINITE;
    if (conv) return NYX_HIP_TGT_OK_CONVERGED;
    double ss = err[0] * err[0];
TGT_UNROLL
    for (int i = 1; i < TGT_MO; ++i)
        if (i < O) ss = ss + err[i] * err[i];
    const double nrm = sqrt(ss);
    if (fabs(nrm - run.prev) < 1e-10) return NYX_HIP_TGT_INEFFECTIVE;
    run.prev = nrm;

    // the Gram matrix (its lower triangle) and the right-hand side: O < V the minimum-norm step, otherwise least squares
    const bool wide = O < V;
    const int m = wide ? O : V;
    double J[TGT_MO][TGT_MV];
TGT_UNROLL
    for (int i = 0; i < TGT_MO; ++i) {
TGT_UNROLL
        for (int j = 0; j < TGT_MV; ++j) J[i][j] = (i < O && j < V) ? park[(int64_t)(i * TGT_MV + j) * ps] : 0.0;
    }
    double L[6][6], b[6];
    if (wide) {
TGT_UNROLL
        for (int a = 0; a < 6; ++a) {
            b[a] = err[a];
TGT_UNROLL
            for (int c = 0; c <= a; ++c) {
                double g = J[a][0] * J[c][0];
TGT_UNROLL
                for (int j = 1; j < TGT_MV; ++j)
                    if (j < V) g = g + J[a][j] * J[c][j];
                L[a][c] = g;
            }
        }
    } else {
TGT_UNROLL
        for (int a = 0; a < 6; ++a) {
            double r = J[0][a] * err[0];
TGT_UNROLL
            for (int i = 1; i < TGT_MO; ++i)
                if (i < O) r = r + J[i][a] * err[i];
            b[a] = r;
TGT_UNROLL
            for (int c = 0; c <= a; ++c) {
                double g = J[0][a] * J[0][c];
TGT_UNROLL
                for (int i = 1; i < TGT_MO; ++i)
                    if (i < O) g = g + J[i][a] * J[i][c];
                L[a][c] = g;
            }
        }
    }
    // unpivoted Cholesky, in place: L L^T = G
    bool singular = false;
TGT_UNROLL
    for (int i = 0; i < 6; ++i)
        if (i < m) {
TGT_UNROLL
            for (int j = 0; j <= i; ++j) {
                double s = L[i][j];
TGT_UNROLL
                for (int k = 0; k < j; ++k) s = s - L[i][k] * L[j][k];
                if (i == j) {
                    singular = !(s > 0.0) || !tgt_finite(s) || singular;
                    L[i][i] = sqrt(s);
                } else {
                    L[i][j] = s / L[j][j];
                }
            }
        }
    if (singular) return NYX_HIP_TGT_SINGULAR;
    double yv[6], xv[6];
TGT_UNROLL
    for (int i = 0; i < 6; ++i) {
        yv[i] = 0.0;
        xv[i] = 0.0;
    }
TGT_UNROLL
    for (int i = 0; i < 6; ++i)
        if (i < m) {
            double s = b[i];
TGT_UNROLL
            for (int k = 0; k < i; ++k) s = s - L[i][k] * yv[k];
            yv[i] = s / L[i][i];
        }
TGT_UNROLL
    for (int i = 5; i >= 0; --i)
        if (i < m) {
            double s = yv[i];
TGT_UNROLL
            for (int k = i + 1; k < 6; ++k)
                if (k < m) s = s - L[k][i] * xv[k];
            xv[i] = s / L[i][i];
        }
    double delta[TGT_MV];
    if (wide) {
TGT_UNROLL
        for (int j = 0; j < TGT_MV; ++j) {
            double d = J[0][j] * xv[0];
TGT_UNROLL
            for (int a = 1; a < TGT_MO; ++a)
                if (a < O) d = d + J[a][j] * xv[a];
            delta[j] = d;
        }
    } else {
TGT_UNROLL
        for (int j = 0; j < TGT_MV; ++j) delta[j] = xv[j];
    }
    // the clamp, on the step: one chain per variable
TGT_UNROLL
    for (int j = 0; j < TGT_MV; ++j) {
        if (j < V) {
            const double ms = fabs(q.var_max_step[j]);
            double d = delta[j];
            if (fabs(d) > ms) d = d > 0.0 ? ms : -ms;
            else if (d > q.var_max_value[j]) d = q.var_max_value[j];
            else if (d < q.var_min_value[j]) d = q.var_min_value[j];
            delta[j] = d;
            run.total[j] = run.total[j] + d;
        } else {
            delta[j] = 0.0;
        }
    }
    double c6[6], frm[6];
    tgt_c6(q, delta, c6);
TGT_UNROLL
    for (int k = 0; k < 6; ++k) frm[k] = frm_at[(int64_t)k * fs];   // (read here, not held through the solve)
    tgt_apply(q.correction_frame, frm, c6, run.xi);   // (in the frame of xi_start, like every step before it: the total is their sum)
    return it >= q.iterations ? NYX_HIP_TGT_TOO_MANY_ITERATIONS : TGT_GOES_ON;
}
