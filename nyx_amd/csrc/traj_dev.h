// traj_dev.h — `Traj::at` on the device: the view of one stored trajectory, HRMINT with its table in registers, and the
// window selection of traj.rs:82-127.  Shared by the trajectory kernels (traj_kernel.hip) and the report kernel
// (report_kernel.hip): both call the SAME code with the same operands, so a sample interpolated for a report is bit-identical
// to the one `nyx_hip_traj_every` / `nyx_hip_traj_at` return for that epoch.  Compile with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/nyx_hip.h"
#include "hifitime_dev.h"

#define DEVFN static __device__ __forceinline__

namespace {

constexpr int LANES = 64;
constexpr int SAMPLES = 13;                 // INTERPOLATION_SAMPLES, interpolatable.rs:22

// The stored states of one trajectory read as the finalize()d (epoch-sorted) sequence (traj.rs:75-80).
struct View {
    const int64_t *epoch;
    int64_t n, i, len;
    bool desc;
    __device__ __forceinline__ int64_t at(int64_t k) const { return (desc ? len - 1 - k : k) * n + i; }
};

DEVFN View make_view(const nyx_hip_traj_t &t, int64_t n, int64_t i) {
    View v;
    v.epoch = t.epoch_ns;
    v.n = n;
    v.i = i;
    const int64_t produced = t.len[i];
    v.len = produced < t.capacity ? produced : t.capacity;
    v.desc = v.len > 1 && t.epoch_ns[(v.len - 1) * n + i] < t.epoch_ns[i];
    return v;
}

// HRMINT for one axis, table in REGISTERS.  The published routine indexes its work array with loop counters; here the
// row loops are unrolled (static register indices) and only the column loop is rolled, so F (function column),
// D (derivative column) and the abscissas never leave the VGPRs.  The updates of one column are independent of each
// other (each reads only entries the column has not overwritten yet) and are issued WITHOUT per-entry branches, so
// the compiler interleaves their division sequences: that instruction-level parallelism is what hides the FP64
// latency at one or two waves per SIMD.  Entry (i, j) exists for i <= 2n - j; the columns are walked in four groups
// of six with static extents 24/18/12/6, the few entries computed beyond the triangle are never read by a valid
// one (their values, possibly inf/NaN, are dead).  The upper abscissa of entry (i, j), xs[(i+j+1)/2 - 1], moves one
// entry to the left per column: XB is shifted, not indexed.  Lanes with fewer than 13 states (short trajectories,
// the 12-state end windows, ns = 0 for lanes without a window) run the same code under selects.
// Returns false on |denominator| < f64::EPSILON (InterpMath, DivisionByZero) in a VALID entry.
template <int EXTENT>
DEVFN void hrmint_columns(int j0, int n2, double x_eval, const double (&XS)[SAMPLES], double (&F)[2 * SAMPLES],
                          double (&D)[2 * SAMPLES], double (&XB)[2 * SAMPLES], bool &bad, double &f, double &df) {
    const double EPS = 2.220446049250313e-16;
#pragma unroll 1
    for (int j = j0; j < j0 + 6; ++j) {
#pragma unroll
        for (int i = 1; i <= EXTENT; ++i) {
            const double xa = XS[(i + 1) / 2 - 1], xb = XB[i];
            const double c1 = xb - x_eval;
            const double c2 = x_eval - xa;
            const double denom = xb - xa;
            bad = bad || (i <= n2 - j && fabs(denom) < EPS);
            D[i - 1] = (c1 * D[i - 1] + c2 * D[i] + (F[i] - F[i - 1])) / denom;
            F[i - 1] = (c1 * F[i - 1] + c2 * F[i]) / denom;
        }
        // a lane whose table ends with this column keeps its result; later columns only touch dead entries
        f = j == n2 - 1 ? F[0] : f;
        df = j == n2 - 1 ? D[0] : df;
#pragma unroll
        for (int i = 1; i <= EXTENT; ++i) XB[i] = XB[i + 1];
    }
}

DEVFN bool hrmint_axis(const double (&XS)[SAMPLES], int ns, double x_eval, const double *py, const double *pv, const View &v,
                       int64_t first_idx, double &f, double &df) {
    const double EPS = 2.220446049250313e-16;
    double F[2 * SAMPLES], D[2 * SAMPLES], XB[2 * SAMPLES];
    bool bad = false;
    const int n2 = 2 * ns;
    // first column: values and derivatives interleaved (rows beyond ns repeat the last state: dead entries)
#pragma unroll
    for (int k = 0; k < SAMPLES; ++k) { F[2 * k] = 0.0; F[2 * k + 1] = 0.0; }
    if (ns > 0) {
#pragma unroll
        for (int k = 0; k < SAMPLES; ++k) {
            const int64_t at = v.at(first_idx + (k < ns ? k : ns - 1));
            F[2 * k] = py[at];
            F[2 * k + 1] = pv[at];
        }
    }
    // second column: first-degree interpolants
#pragma unroll
    for (int i = 1; i <= SAMPLES - 1; ++i) {
        const bool valid = i <= ns - 1;
        const double xa = XS[i - 1], xb = XS[i];
        const double c1 = xb - x_eval;
        const double c2 = x_eval - xa;
        const double denom = xb - xa;
        bad = bad || (valid && fabs(denom) < EPS);
        const double wp = F[2 * i - 2], wc = F[2 * i - 1], wn = F[2 * i];
        D[2 * i - 2] = wc;
        D[2 * i - 1] = (wn - wp) / denom;
        const double temp = wc * (x_eval - xa) + wp;
        F[2 * i - 1] = valid ? (c1 * wp + c2 * wn) / denom : wc;
        F[2 * i - 2] = valid ? temp : wp;
    }
    D[2 * SAMPLES - 2] = 0.0; D[2 * SAMPLES - 1] = 0.0;
#pragma unroll
    for (int k = 0; k < SAMPLES; ++k) {
        const bool last = k == ns - 1;
        D[2 * k] = last ? F[2 * k + 1] : D[2 * k];
        F[2 * k] = last ? F[2 * k + 1] * (x_eval - XS[k]) + F[2 * k] : F[2 * k];
    }
    // columns 3 .. 2n
    XB[0] = 0.0; XB[2 * SAMPLES - 1] = 0.0;
#pragma unroll
    for (int i = 1; i <= 2 * SAMPLES - 2; ++i) XB[i] = XS[(i + 3) / 2 - 1];
    f = F[0];   // n = 1: the table is complete already
    df = D[0];
    hrmint_columns<24>(2, n2, x_eval, XS, F, D, XB, bad, f, df);
    hrmint_columns<18>(8, n2, x_eval, XS, F, D, XB, bad, f, df);
    hrmint_columns<12>(14, n2, x_eval, XS, F, D, XB, bad, f, df);
    hrmint_columns<6>(20, n2, x_eval, XS, F, D, XB, bad, f, df);
    return !bad;
}

// `Traj::at` for the trajectory of this lane.
// `ill` (optional): set when the window of an interpolated sample holds two states closer than 1e-4 of its mean spacing (see
// NYX_HIP_INTERP_ILL_CONDITIONED); the sample itself is the reference's either way.
DEVFN int traj_at(const nyx_hip_traj_t &src, const View &v, int64_t epoch_ns, double s6[6], bool *ill = nullptr) {
    if (ill) *ill = false;
    const double qnan = __builtin_nan("");
    for (int c = 0; c < 6; ++c) s6[c] = qnan;
    int st = NYX_HIP_INTERP_OK;
    int64_t hit = -1, first_idx = 0;
    int ns = 0;
    if (v.len == 0 || v.epoch[v.at(0)] > epoch_ns || v.epoch[v.at(v.len - 1)] < epoch_ns) {
        st = NYX_HIP_INTERP_NO_DATA;
    } else {
        // binary search (traj.rs:88-91): exact hit, or the insertion index
        int64_t lo = 0, hi = v.len;
        while (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            const int64_t e = v.epoch[v.at(mid)];
            if (e == epoch_ns) { hit = mid; break; }
            if (e < epoch_ns) lo = mid + 1; else hi = mid;
        }
        if (hit < 0) {
            const int64_t idx = lo;
            if (idx == 0 || idx >= v.len) {
                st = NYX_HIP_INTERP_NO_DATA;
            } else {
                const int64_t num_left = SAMPLES / 2;
                first_idx = idx > num_left ? idx - num_left : 0;
                const int64_t last_idx = v.len < first_idx + SAMPLES ? v.len : first_idx + SAMPLES;
                if (last_idx == v.len) first_idx = last_idx > 2 * num_left ? last_idx - 2 * num_left : 0;  // 12 states, sic
                ns = (int)(last_idx - first_idx);
            }
        }
    }
    if (hit >= 0) {
        const int64_t at = v.at(hit);
        s6[0] = src.x_km[at]; s6[1] = src.y_km[at]; s6[2] = src.z_km[at];
        s6[3] = src.vx_km_s[at]; s6[4] = src.vy_km_s[at]; s6[5] = src.vz_km_s[at];
    }
    // the interpolation proper: lanes without a window carry ns = 0 and fall through every predicate
    if (__any(ns > 0)) {
        double XS[SAMPLES];
#pragma unroll
        for (int k = 0; k < SAMPLES; ++k) XS[k] = k < ns ? ns_to_seconds(v.epoch[v.at(first_idx + k)]) : 0.0;
        const double x_eval = ns_to_seconds(epoch_ns);
        if (ill && ns > 1) {
            double dmin = fabs(XS[1] - XS[0]);
#pragma unroll
            for (int k = 2; k < SAMPLES; ++k)
                if (k < ns) dmin = fmin(dmin, fabs(XS[k] - XS[k - 1]));
            *ill = dmin < 1e-4 * (fabs(XS[ns - 1] - XS[0]) / (double)(ns - 1));
        }
        bool ok = true;
        double fx = qnan, fy = qnan, fz = qnan, dx = qnan, dy = qnan, dz = qnan;
#pragma unroll 1
        for (int c = 0; c < 3; ++c) {
            const double *py = c == 0 ? src.x_km : (c == 1 ? src.y_km : src.z_km);
            const double *pv = c == 0 ? src.vx_km_s : (c == 1 ? src.vy_km_s : src.vz_km_s);
            double f, df;
            ok = hrmint_axis(XS, ns, x_eval, py, pv, v, first_idx, f, df) && ok;
            if (c == 0) { fx = f; dx = df; } else if (c == 1) { fy = f; dy = df; } else { fz = f; dz = df; }
        }
        if (ns > 0) {
            if (ok) { s6[0] = fx; s6[1] = fy; s6[2] = fz; s6[3] = dx; s6[4] = dy; s6[5] = dz; }
            else st = NYX_HIP_INTERP_MATH;
        }
    }
    return st;
}

}  // namespace
