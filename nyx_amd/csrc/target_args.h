// target_args.h — launch arguments of the targeter kernels (target_kernel.hip), shared with abi.cpp, and what the two entries of
// include/nyx_hip_target.h refuse before anything is launched (host and device text; no HIP).  The refusals are data (Refusal,
// refusal.h) and are tested on the CPU (tests/test_target_abi.py through the C entries, tests/cxx/target_host_check.cpp directly).
// Last, the device block of the host flavour's outputs and the result bound into it (the same program).
#pragma once
#include <stdint.h>

#include <cmath>

#include "../../include/nyx_hip_target.h"
#include "batch_bind.h"    // kStateRow
#include "chain_args.h"    // Refusal, bad_arg, ResolvedChain
#include "dev_block.h"
#include "devcfg.h"
#include "frame_args.h"    // frm_param_needs

// What a run keeps between the iterations, one row of `cap` doubles each (TgtArgs.keep + row * cap + i)
enum { TGT_XI_START = 0, TGT_XI = 6, TGT_TOTAL = 12, TGT_PREV = 18, TGT_PARK = 19 /* the Jacobian of the round, 36 rows */, TGT_KEEP_ROWS = 55 };
// TgtArgs.flag[i]
enum { TGT_RUN_ACTIVE = 0, TGT_RUN_ENDED = 1, TGT_RUN_LEG_FAILED = 2 };

// The rows of a batch as the kernels walk them: the epoch, the thirteen double rows of nyx_hip_states_t in header order (a row the
// caller left out is NULL and is neither read nor written), the propagation status
struct TgtRows {
    int64_t *epoch;
    double *f[13];
    int32_t *status;
};

struct TgtArgs {
    nyx_hip_target_query_t q;
    int64_t n;          // runs
    int64_t cap;        // row length of `keep`
    TgtRows start;      // [n] the runs at the correction epoch (the first launch's outputs), with that launch's status
    TgtRows work;       // [(1 + V) n] row k n + i: k = 0 the nominal, k = 1 .. V the perturbed states; propagated in place
    double *keep;       // [TGT_KEEP_ROWS][cap]
    int32_t *flag;      // [n] TGT_RUN_*
    int32_t *active;    // [iterations + 2] runs still active after round `it`
    int32_t it;         // the round of this launch of the step kernel
    int32_t need;       // tgt_needs(q): FRM_NEED_* | REP_NEED_* of the objectives, filled by the launcher
    ResolvedChain chain;   // the objective target's chain, resolved against the context's segment rows by the launcher
    const double *records;   // the context's ephemeris records on the device (DevSeg.offset points into it)
    // outputs
    int32_t *o_status, *o_iterations;
    double *o_correction, *o_errors;
    TgtRows corrected, achieved;   // (their status pointers are unused)
};
static_assert(sizeof(TgtArgs) <= 4096, "TgtArgs must fit the kernel-argument segment");

inline TgtRows tgt_rows(const nyx_hip_states_t &s, int32_t *status) {
    return TgtRows{s.epoch_ns, {s.x_km, s.y_km, s.z_km, s.vx_km_s, s.vy_km_s, s.vz_km_s, s.cr, s.cd, s.prop_mass_kg, s.dry_mass_kg, s.extra_mass_kg,
                                s.srp_area_m2, s.drag_area_m2}, status};
}

// FRM_NEED_* | REP_NEED_* of the objectives of a query check_target has accepted
static inline int32_t tgt_needs(const nyx_hip_target_query_t &q) {
    int32_t need = 0;
    for (int i = 0; i < q.n_objs; ++i) need |= frm_param_needs(q.obj_param[i]);
    return need;
}

// ---- refusals, in the order of the header's list.  check_target never dereferences the context; check_target_context is what the
// query asks of it (of a query the first accepted)
inline bool tgt_has_rows(const nyx_hip_states_t &s) { return s.epoch_ns && s.x_km && s.y_km && s.z_km && s.vx_km_s && s.vy_km_s && s.vz_km_s; }

inline Refusal check_target(const nyx_hip_ctx *ctx, const nyx_hip_states_t *in, const nyx_hip_target_query_t *q, const nyx_hip_target_result_t *res) {
    const char *name = "target_batch";
    if (!ctx) return bad_arg("null ctx");
    if (!q) return bad_arg("%s: null query", name);
    if (!res) return bad_arg("%s: null result", name);
    if (q->n_vars < 1 || q->n_vars > NYX_HIP_MAX_TARGET_VARS) return bad_arg("%s: n_vars = %d, 1 .. %d variables", name, q->n_vars, NYX_HIP_MAX_TARGET_VARS);
    if (q->n_objs < 1 || q->n_objs > NYX_HIP_MAX_TARGET_OBJS) return bad_arg("%s: n_objs = %d, 1 .. %d objectives", name, q->n_objs, NYX_HIP_MAX_TARGET_OBJS);
    if (q->iterations < 0 || q->iterations > NYX_HIP_TARGET_MAX_ITERATIONS)
        return bad_arg("%s: iterations = %d, 0 .. %d", name, q->iterations, NYX_HIP_TARGET_MAX_ITERATIONS);
    if (q->correction_frame != NYX_HIP_FRAME_INERTIAL && q->correction_frame != NYX_HIP_FRAME_VNC)
        return bad_arg("%s: correction_frame = %d, inertial (0) or VNC (2)", name, q->correction_frame);
    for (int j = 0; j < q->n_vars; ++j) {
        if (q->var_component[j] < 0 || q->var_component[j] >= NYX_HIP_VARY_COUNT)
            return bad_arg("%s: var_component[%d] = %d is not a nyx_hip_target_vary", name, j, q->var_component[j]);
        if (!(std::isfinite(q->var_perturbation[j]) && q->var_perturbation[j] != 0.0)) return bad_arg("%s: var_perturbation[%d] must be finite and not zero", name, j);
        if (!std::isfinite(q->var_init_guess[j])) return bad_arg("%s: var_init_guess[%d] must be finite", name, j);
        if (!(q->var_max_step[j] >= 0.0)) return bad_arg("%s: var_max_step[%d] must be >= 0", name, j);
        if (!(q->var_max_value[j] >= 0.0)) return bad_arg("%s: var_max_value[%d] must be >= 0", name, j);
        if (!(q->var_min_value[j] <= q->var_max_value[j])) return bad_arg("%s: var_min_value[%d] must be <= var_max_value[%d]", name, j, j);
        if (q->correction_frame == NYX_HIP_FRAME_VNC && q->var_component[j] < NYX_HIP_VARY_VELOCITY_X)
            return bad_arg("%s: var_component[%d] is a position: a correction frame takes velocity variables only", name, j);
    }
    for (int o = 0; o < q->n_objs; ++o) {
        if (frm_param_needs(q->obj_param[o]) < 0) return bad_arg("%s: obj_param[%d] = %d is not a nyx_hip_frame_param", name, o, q->obj_param[o]);
        if (!(std::isfinite(q->obj_tolerance[o]) && q->obj_tolerance[o] >= 0.0)) return bad_arg("%s: obj_tolerance[%d] must be finite and >= 0", name, o);
        if (!std::isfinite(q->obj_desired[o]) || !std::isfinite(q->obj_mult[o]) || !std::isfinite(q->obj_add[o]))
            return bad_arg("%s: obj_desired[%d], obj_mult[%d] and obj_add[%d] must be finite", name, o, o, o);
    }
    if (Refusal r = check_chain(name, "", chain_view(*q), 0)) return r;
    if (!(std::isfinite(q->mu_km3_s2) && q->mu_km3_s2 > 0.0)) return bad_arg("%s: mu_km3_s2 must be finite and > 0", name);
    if (!in || in->n < 0 || !tgt_has_rows(*in)) return bad_arg("%s: in: epoch and the six Cartesian arrays are mandatory", name);
    if (!res->status || !res->iterations || !res->correction || !res->achieved_errors)
        return bad_arg("%s: status, iterations, correction and achieved_errors arrays required", name);
    if (!tgt_has_rows(res->corrected) || !tgt_has_rows(res->achieved))
        return bad_arg("%s: corrected and achieved: epoch and the six Cartesian arrays are mandatory", name);
    if (in->stm) {
        Refusal r = bad_arg("%s: in->stm is given: the hyperdual targeter is not on the device path", name);
        r.rc = NYX_HIP_RC_UNSUPPORTED;
        return r;
    }
    return {};
}

inline Refusal check_target_context(const nyx_hip_target_query_t &q, int n_seg, bool carries_stm, bool frame_swapped) {
    const char *name = "target_batch";
    if (Refusal r = check_chain_context(name, "", chain_view(q), n_seg)) return r;
    if (carries_stm) {
        Refusal r = bad_arg("%s: the context carries STMs: the hyperdual targeter is not on the device path", name);
        r.rc = NYX_HIP_RC_UNSUPPORTED;
        return r;
    }
    if (frame_swapped) return frame_swap_refusal(name, "its chains are not those of the states it integrates");
    return {};
}

// ---- the device block of the host flavour's outputs (Block<N>, dev_block.h): correction [V][n], errors [O][n], corrected and achieved
// (one epoch row, then the thirteen double rows of nyx_hip_states_t in header order, of n each), status [n], iterations [n]
enum { TGB_CORRECTION, TGB_ERRORS, TGB_CORRECTED, TGB_ACHIEVED, TGB_STATUS, TGB_ITERATIONS, TGB_PARTS };
inline Block<TGB_PARTS> target_block(int64_t n, int n_vars, int n_objs) {
    const size_t row = (size_t)n * sizeof(double), words = (size_t)n * sizeof(int32_t);
    return Block<TGB_PARTS>({n_vars * row, n_objs * row, (1 + kStateRows) * row, (1 + kStateRows) * row, words, words});
}
// row k of the part TGB_CORRECTED or TGB_ACHIEVED: k = 0 the epochs, k = 1 + r the state row r (kStateRow, batch_bind.h)
inline Part target_row(const Block<TGB_PARTS> &b, int part, int k) {
    const size_t row = b[part].bytes / (1 + kStateRows);
    return {b[part].at + k * row, row};
}
// The pointers of `d` into a block at `base` (every row of both states is there, whichever rows the caller wants back).
inline void bind_target_result(nyx_hip_target_result_t &d, char *base, const Block<TGB_PARTS> &b) {
    d.correction = (double *)(base + b[TGB_CORRECTION].at);
    d.achieved_errors = (double *)(base + b[TGB_ERRORS].at);
    d.status = (int32_t *)(base + b[TGB_STATUS].at);
    d.iterations = (int32_t *)(base + b[TGB_ITERATIONS].at);
    nyx_hip_states_t *views[2] = {&d.corrected, &d.achieved};
    for (int s = 0; s < 2; ++s) {
        views[s]->n = (int64_t)(b[TGB_STATUS].bytes / sizeof(int32_t));
        views[s]->epoch_ns = (int64_t *)(base + target_row(b, TGB_CORRECTED + s, 0).at);
        for (int k = 0; k < kStateRows; ++k) views[s]->*kStateRow[k].s = (double *)(base + target_row(b, TGB_CORRECTED + s, 1 + k).at);
    }
}
