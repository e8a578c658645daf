// lambert_args.h — launch arguments of the Lambert kernels (lambert_kernel.hip), shared with abi.cpp, and what the two entries of
// include/nyx_hip_lambert.h refuse before anything is launched (host and device text; no HIP).  The refusals are data (Refusal,
// refusal.h) and are tested on the CPU (tests/test_lambert_abi.py through the C entries).  The three chains of a grid are
// ResolvedChains (chain_args.h).  Last, the device blocks of the two host flavours (tests/cxx/lambert_host_check.cpp).
#pragma once
#include <stdint.h>

#include <cmath>

#include "../../include/nyx_hip_lambert.h"
#include "chain_args.h"   // Refusal, bad_arg, ResolvedChain
#include "dev_block.h"
#include "devcfg.h"

struct LmbBatchArgs {
    const double *rv1, *rv2, *tof_s;  // device pointers, component-major [c * n + i]
    int64_t n;
    double mu;
    nyx_hip_lambert_query_t q;
    double *values;    // [n_params][n]
    int32_t *status;   // [n]
};

struct LmbGridArgs {
    nyx_hip_lambert_grid_query_t q;
    const double *records;   // the context's ephemeris records on the device (DevSeg.offset points into it)
    ResolvedChain dep, arr, centre;   // filled by the launcher (resolve_chain)
    double *values;    // [n_params][n_dep][n_arr]
    int32_t *status;   // [n_dep][n_arr]
};
static_assert(sizeof(LmbGridArgs) <= 4096, "LmbGridArgs must fit the kernel-argument segment");

// ---- refusals.  The solver's settings first, in the order of the header's list
inline Refusal check_lambert_query(const char *name, const nyx_hip_ctx *ctx, const nyx_hip_lambert_query_t *q, double mu_km3_s2) {
    if (!ctx) return bad_arg("null ctx");
    if (!q) return bad_arg("%s: null query", name);
    if (q->n_params < 1 || q->n_params > NYX_HIP_MAX_LAMBERT_PARAMS)
        return bad_arg("%s: n_params = %d, 1 .. %d parameters per call", name, q->n_params, NYX_HIP_MAX_LAMBERT_PARAMS);
    for (int p = 0; p < q->n_params; ++p)
        if (q->param[p] < 0 || q->param[p] >= NYX_HIP_LMB_COUNT) return bad_arg("%s: param[%d] = %d is not a nyx_hip_lambert_param", name, p, q->param[p]);
    if (q->way < 0 || q->way >= NYX_HIP_LMB_WAY_COUNT) return bad_arg("%s: way = %d is not a nyx_hip_lambert_way", name, q->way);
    if (q->n_revs < 0 || q->n_revs > NYX_HIP_LMB_MAX_REVS) return bad_arg("%s: n_revs = %d, 0 .. %d", name, q->n_revs, NYX_HIP_LMB_MAX_REVS);
    if (q->high_path != 0 && q->high_path != 1) return bad_arg("%s: high_path = %d, 0 or 1", name, q->high_path);
    if (!(q->tol >= NYX_HIP_LMB_TOL_MIN && q->tol <= NYX_HIP_LMB_TOL_MAX)) return bad_arg("%s: tol = %g, 1e-13 .. 1e-2", name, q->tol);
    if (q->max_iter < 1 || q->max_iter > NYX_HIP_LMB_MAX_ITER) return bad_arg("%s: max_iter = %d, 1 .. %d", name, q->max_iter, NYX_HIP_LMB_MAX_ITER);
    if (!(std::isfinite(mu_km3_s2) && mu_km3_s2 > 0.0)) return bad_arg("%s: mu_km3_s2 must be finite and > 0", name);
    return {};
}

inline Refusal check_lambert_batch(const nyx_hip_ctx *ctx, const double *rv1, const double *rv2, const double *tof_s, int64_t n, double mu_km3_s2,
                                   const nyx_hip_lambert_query_t *q, const double *values, const int32_t *status) {
    const char *name = "lambert_batch";
    if (Refusal r = check_lambert_query(name, ctx, q, mu_km3_s2)) return r;
    if (n < 0) return bad_arg("negative n");
    if (!rv1 || !rv2 || !tof_s) return bad_arg("%s: rv1, rv2 and tof_s arrays required", name);
    if (!values || !status) return bad_arg("%s: values and status arrays required", name);
    return {};
}

inline bool lmb_same_chain(const nyx_hip_lambert_chain_t &a, const nyx_hip_lambert_chain_t &b) {
    if (a.n_chain != b.n_chain) return false;
    for (int k = 0; k < a.n_chain; ++k)
        if (a.chain_segment[k] != b.chain_segment[k] || a.chain_sign[k] != b.chain_sign[k]) return false;
    return true;
}

// check_lambert_grid never dereferences the context; check_lambert_context is what the query asks of it (of a query the first accepted)
inline Refusal check_lambert_grid(const nyx_hip_ctx *ctx, const nyx_hip_lambert_grid_query_t *q, const double *values, const int32_t *status) {
    const char *name = "lambert_grid";
    if (!ctx) return bad_arg("null ctx");
    if (!q) return bad_arg("%s: null query", name);
    if (Refusal r = check_lambert_query(name, ctx, &q->solve, q->mu_km3_s2)) return r;
    if (q->n_dep < 0 || q->n_arr < 0 || q->n_dep > INT32_MAX || q->n_arr > INT32_MAX)
        return bad_arg("%s: n_dep = %lld, n_arr = %lld, 0 .. 2^31 - 1 each", name, (long long)q->n_dep, (long long)q->n_arr);
    if (q->has_tof != 0 && q->has_tof != 1) return bad_arg("%s: has_tof = %d, 0 or 1", name, q->has_tof);
    if (q->dep_step_ns <= 0) return bad_arg("%s: dep_step_ns must be > 0", name);
    if (q->has_tof ? q->tof_step_ns <= 0 : q->arr_step_ns <= 0) return bad_arg("%s: %s must be > 0", name, q->has_tof ? "tof_step_ns" : "arr_step_ns");
    if (!values || !status) return bad_arg("%s: values and status arrays required", name);
    if (Refusal r = check_chain(name, "dep", chain_view(q->dep), 0)) return r;
    if (Refusal r = check_chain(name, "arr", chain_view(q->arr), 0)) return r;
    if (Refusal r = check_chain(name, "centre", chain_view(q->centre), 0)) return r;
    if (lmb_same_chain(q->dep, q->centre)) return bad_arg("%s: the departure body's chain is the centre's: its radius is zero by construction", name);
    if (lmb_same_chain(q->arr, q->centre)) return bad_arg("%s: the arrival body's chain is the centre's: its radius is zero by construction", name);
    return {};
}
inline Refusal check_lambert_context(const nyx_hip_lambert_grid_query_t &q, int n_seg, bool frame_swapped) {
    const char *name = "lambert_grid";
    if (Refusal r = check_chain_context(name, "dep", chain_view(q.dep), n_seg)) return r;
    if (Refusal r = check_chain_context(name, "arr", chain_view(q.arr), n_seg)) return r;
    if (Refusal r = check_chain_context(name, "centre", chain_view(q.centre), n_seg)) return r;
    if (frame_swapped) return frame_swap_refusal(name, "its chains are not those of the states it integrates");   // NYX_HIP_RC_UNSUPPORTED
    return {};
}

// ---- the device blocks of the two host flavours (Block<N>, dev_block.h).  A batch: rv1 [6][n], rv2 [6][n], tof_s [n], values
// [n_params][n], status [n]; a grid: values [n_params][n_dep][n_arr], status [n_dep][n_arr]
enum { LBB_RV1, LBB_RV2, LBB_TOF, LBB_VALUES, LBB_STATUS, LBB_PARTS };
inline Block<LBB_PARTS> lambert_batch_block(int64_t n, int n_params) {
    const size_t row = (size_t)n * sizeof(double);
    return Block<LBB_PARTS>({6 * row, 6 * row, row, (size_t)n_params * row, (size_t)n * sizeof(int32_t)});
}
enum { LGB_VALUES, LGB_STATUS, LGB_PARTS };
inline Block<LGB_PARTS> lambert_grid_block(int64_t n_dep, int64_t n_arr, int n_params) {
    const size_t cells = (size_t)n_dep * (size_t)n_arr;
    return Block<LGB_PARTS>({(size_t)n_params * cells * sizeof(double), cells * sizeof(int32_t)});
}
