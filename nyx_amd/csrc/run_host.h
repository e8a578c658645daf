// run_host.h - the host side of the entries that run the propagator and of the two older host flavours (host only, no HIP; abi.cpp,
// tests/cxx/run_host_check.cpp): what they refuse, in the order the checks fire; the device blocks of predict_until, until_event and
// ensemble_moments (Block<N>, dev_block.h); the segments of a covariance-mapping loop.  (Their launch predicates: launch_plan.h, beside pick_quad.)
#pragma once
#include <algorithm>

#include "dev_block.h"
#include "predict_args.h"
#include "series_host.h"  // Refusal, bad_arg, check_traj, check_traj_eval

inline Refusal unsupported(Refusal r) { r.rc = NYX_HIP_RC_UNSUPPORTED; return r; }  // (the message of a bad_arg, the other code)
inline bool has_cartesian(const nyx_hip_states_t &s) { return s.x_km && s.y_km && s.z_km && s.vx_km_s && s.vy_km_s && s.vz_km_s; }
inline Refusal check_states(const nyx_hip_states_t *s, const char *what) {
    return !s || s->n < 0 || !s->epoch_ns || !has_cartesian(*s) ? bad_arg("%s: epoch and the six Cartesian arrays are mandatory", what) : Refusal();
}

// What the host bracket of a run (host_run, abi.cpp) checks after the entry's own checks; an accepted batch with in->n == 0 is done
// (check_states leaves no out->n below it).  `need_stm`: the STMs are uploaded (an STM context; not predict_until: identity).
inline Refusal check_run(const nyx_hip_ctx *ctx, const nyx_hip_states_t *in, const nyx_hip_states_t *out, bool need_stm) {
    if (!ctx) return bad_arg("null ctx");
    if (Refusal r = check_states(in, "in")) return r;
    if (Refusal r = check_states(out, "out")) return r;
    if (out->n < in->n) return bad_arg("out batch smaller than in batch");
    if (in->n > 0 && need_stm && (!in->stm || !out->stm)) return bad_arg("STM context: in->stm and out->stm are mandatory");
    return {};
}
// (propagate_batch_with_traj, and propagate_batch_sharded when it is given one)
inline Refusal check_traj_wanted(const nyx_hip_traj_t *traj) { return !traj || traj->capacity < 1 ? bad_arg("traj with capacity >= 1 required") : Refusal(); }
inline Refusal check_sharded(nyx_hip_ctx *const *ctxs, int32_t n_ctx, const nyx_hip_states_t *in, const nyx_hip_states_t *out, const nyx_hip_traj_t *traj) {
    if (!ctxs || n_ctx < 1 || !in || !out) return bad_arg("sharded: null argument or no context");
    for (int32_t k = 0; k < n_ctx; ++k)
        if (!ctxs[k]) return bad_arg("sharded: null context %d", k);
    if (out->n != in->n) return bad_arg("sharded: out->n != in->n");
    return traj ? check_traj_wanted(traj) : Refusal();
}

inline Refusal check_event(const nyx_hip_ctx *ctx, const nyx_hip_event_t *event, const nyx_hip_traj_t *traj) {
    if (!ctx || !event) return bad_arg("until_event: ctx and event are mandatory");
    if (event->has_frame && (event->frame.kind != NYX_HIP_ROT_IAU || event->frame.n_nut_prec < 0 || event->frame.n_nut_prec > NYX_HIP_MAX_NUT_PREC))
        return unsupported(bad_arg("until_event: the event frame must be an IAU-oriented frame (NYX_HIP_ROT_IAU)"));
    if ((event->scalar == NYX_HIP_EV_LATITUDE_DEG || event->scalar == NYX_HIP_EV_HEIGHT_KM) &&
        !(event->frame_eq_radius_km > 0.0 && event->frame_flattening >= 0.0 && event->frame_flattening < 1.0))
        return bad_arg("until_event: geodetic scalars need the frame's ellipsoid (frame_eq_radius_km > 0, 0 <= flattening < 1)");
    if (event->scalar < NYX_HIP_EV_TRUE_ANOMALY_DEG || event->scalar > NYX_HIP_EV_HEIGHT_KM || event->trigger < 1 ||
        event->epoch_precision_ns < 0 || !(event->value_precision >= 0.0))
        return bad_arg("until_event: bad event (scalar, trigger >= 1, precisions >= 0)");
    if (Refusal r = check_traj(traj, "traj", true)) return r;
    if (traj->capacity < 2) return bad_arg("until_event: traj->capacity >= 2 required (the search needs the bracket)");
    return {};
}
// `flags`: the context's (DevCfg.flags; not read without a context)
inline Refusal check_predict(const nyx_hip_ctx *ctx, uint32_t flags, const nyx_hip_predict_t *cfg, const nyx_hip_estimates_t *est, const nyx_hip_predict_history_t *hist) {
    if (!ctx || !cfg || !est || !est->covar) return bad_arg("predict: ctx, cfg and est->covar are mandatory");
    if (!(flags & NYX_HIP_FLAG_STM)) return bad_arg("predict: the context must be created with NYX_HIP_FLAG_STM");
    if (cfg->max_step_ns <= 0) return bad_arg("predict: max_step_ns must be > 0");
    if (cfg->n_process_noise < 0 || cfg->n_process_noise > NYX_HIP_MAX_PROCESS_NOISE) return bad_arg("predict: n_process_noise out of range");
    for (int q = 0; q < cfg->n_process_noise; ++q)
        if (cfg->process_noise[q].local_frame < NYX_HIP_FRAME_INERTIAL || cfg->process_noise[q].local_frame > NYX_HIP_FRAME_VNC)
            return unsupported(bad_arg("predict: process noise %d: local frame not on the device path (inertial, RIC, VNC)", q));
    if (hist && (hist->capacity < 0 || !hist->n_updates)) return bad_arg("predict: hist->n_updates is mandatory, capacity >= 0");
    return {};
}
// ensemble_moments: the device flavour (one check) and the host flavour (two: it stages the arrays, then runs the device flavour on the copy)
inline Refusal check_moments(const nyx_hip_ctx *ctx, const nyx_hip_states_t *s, const double *out55, bool host) {
    const bool given = ctx && s && out55 && s->n >= 0;
    if (host && !given) return bad_arg("ensemble_moments: null argument");
    if (given && (s->n == 0 || has_cartesian(*s))) return {};
    return bad_arg(host ? "ensemble_moments: the six Cartesian arrays are mandatory" : "ensemble_moments: ctx, states (six Cartesian arrays) and out are mandatory");
}
// The host flavour of traj_at / traj_every: the device flavour's checks, but an empty batch is done whatever the query (m, step_ns).
inline Refusal check_traj_eval_host(const nyx_hip_ctx *ctx, const nyx_hip_traj_t *traj, int64_t n, const int64_t *query, int64_t m, int64_t step_ns, const nyx_hip_traj_t *out, const int32_t *status, int mode) {
    return check_traj_eval(ctx, traj, n, query, n ? m : 0, n ? step_ns : 1, out, status, mode);
}

// ---- the device blocks (Block<N>, dev_block.h)
// predict_until: the covariances [n][81], the six int64 work rows [n], the deviations [n][9], the history arrays the caller asks for
// (widths 1, 9, 81, 81, 9 per slot, capacity * n slots; contiguous, behind the deviations: cleared in one piece), status, n_updates [n]
enum { P_COVAR, P_PREV_EPOCH, P_DUR, P_ACC_N_ACC, P_ACC_N_REJ, P_ACC_N_EVALS, P_INIT_EPOCH, P_SDEV, P_H_EPOCH, P_H_STATE, P_H_STM, P_H_COVAR, P_H_SDEV, P_STATUS, P_N_UPDATES, P_COUNT };
inline Block<P_COUNT> predict_block(int64_t n, const nyx_hip_predict_history_t &h) {
    const size_t row = (size_t)n * 8, words = (size_t)n * 4, slot = (size_t)h.capacity * row;
    return Block<P_COUNT>({81 * row, row, row, row, row, row, row, 9 * row, h.epoch_ns ? slot : 0, h.state ? 9 * slot : 0, h.stm ? 81 * slot : 0,
                           h.covar ? 81 * slot : 0, h.state_dev ? 9 * slot : 0, words, words});
}
// The pointers of `a` into a block at `base` (a history array not asked for: null).
inline void bind_predict(PredictArgs &a, char *base, const Block<P_COUNT> &b) {
    auto at = [&](int k) { return b[k].bytes ? base + b[k].at : nullptr; };
    a.covar = (double *)at(P_COVAR); a.state_dev = (double *)at(P_SDEV); a.status = (int32_t *)at(P_STATUS); a.hist.n_updates = (int32_t *)at(P_N_UPDATES);
    a.prev_epoch = (int64_t *)at(P_PREV_EPOCH); a.dur = (int64_t *)at(P_DUR); a.init_epoch = (int64_t *)at(P_INIT_EPOCH);
    a.acc_n_acc = (int64_t *)at(P_ACC_N_ACC); a.acc_n_rej = (int64_t *)at(P_ACC_N_REJ); a.acc_n_evals = (int64_t *)at(P_ACC_N_EVALS);
    a.hist.epoch_ns = (int64_t *)at(P_H_EPOCH); a.hist.state = (double *)at(P_H_STATE); a.hist.stm = (double *)at(P_H_STM);
    a.hist.covar = (double *)at(P_H_COVAR); a.hist.state_dev = (double *)at(P_H_SDEV);
}

// until_event: the previous value of the scalar [n] (f64), then the crossings counted and the found flags [n] (i32)
enum { E_PREV, E_COUNT, E_FOUND, E_PARTS };
inline Block<E_PARTS> event_block(int64_t n) { return Block<E_PARTS>({(size_t)n * 8, (size_t)n * 4, (size_t)n * 4}); }
// ensemble_moments (host flavour): nine rows [n] (a row the caller leaves null keeps its place), then the status words [n]
enum { M_STATUS = 9, M_PARTS };
inline Block<M_PARTS> moments_block(int64_t n, bool status_given) {
    const size_t row = (size_t)n * 8;
    return Block<M_PARTS>({row, row, row, row, row, row, row, row, row, status_given ? (size_t)n * 4 : 0});
}

// ---- segments a covariance-mapping loop needs: the longest trajectory decides (the others idle with duration 0), one at least
// (spans are assumed to fit an int64, as they always were)
inline int64_t predict_segments(const int64_t *epoch_ns, int64_t n, int64_t end_epoch_ns, int64_t max_step_ns) {
    int64_t n_seg = 1;
    for (int64_t i = 0; i < n; ++i)
        if (end_epoch_ns > epoch_ns[i]) n_seg = std::max(n_seg, (end_epoch_ns - epoch_ns[i] + max_step_ns - 1) / max_step_ns);
    return n_seg;
}
