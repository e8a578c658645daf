// series_host.h - the host side of the sampled-series entries (host only, no HIP; abi.cpp, the launchers of the eight series kernels,
// tests/cxx/series_host_check.cpp): what traj_at / traj_every and the seven fused reports (values, ground track, station views, eclipses, encounters, RIC, links) refuse, the
// one output block of a report's host flavour (a Block<N>, dev_block.h), and the chunks of consecutive samples a launch cuts a span into.
#pragma once
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "aer_args.h"
#include "chain_args.h"   // Refusal, bad_arg (refusal.h), check_chain, check_chain_context, frame_swap_refusal
#include "dev_block.h"
#include "eclipse_args.h"
#include "frame_args.h"
#include "groundtrack_args.h"
#include "link_args.h"
#include "report_args.h"
#include "ric_args.h"
#include "traj_args.h"

inline Refusal check_traj(const nyx_hip_traj_t *t, const char *what, bool need_epochs) {
    if (!t || t->capacity < 0 || !t->len || !t->x_km || !t->y_km || !t->z_km || !t->vx_km_s || !t->vy_km_s || !t->vz_km_s ||
        (need_epochs && !t->epoch_ns))
        return bad_arg("%s: null array or negative capacity", what);
    return {};
}

// traj_at / traj_every on device arrays (mode = TRAJ_MODE_*)
inline Refusal check_traj_eval(const nyx_hip_ctx *ctx, const nyx_hip_traj_t *traj, int64_t n, const int64_t *query, int64_t m,
                               int64_t step_ns, const nyx_hip_traj_t *out, const int32_t *status, int mode) {
    if (!ctx) return bad_arg("null ctx");
    if (Refusal r = check_traj(traj, "traj", true)) return r;
    if (Refusal r = check_traj(out, "out", true)) return r;
    if (n < 0) return bad_arg("negative n");
    if (mode == TRAJ_MODE_AT) {
        if (m < 0 || (m > 0 && (!query || !status))) return bad_arg("traj_at: query/status arrays required");
        if (out->capacity < m) return bad_arg("traj_at: out->capacity < m");
    } else if (step_ns <= 0) {
        return bad_arg("traj_every: step_ns must be > 0 (TimeSeries with a positive step)");
    }
    return {};
}

// ---- what every series query (`name`: the entry, as the messages call it) is checked for, in the order the checks fire: the
// opening (RIC: with its reference), the entry's own first checks, the step and the capacity, its own later checks, the outputs
inline Refusal series_open(const char *name, const nyx_hip_ctx *ctx, const nyx_hip_traj_t *traj, bool with_ref, const nyx_hip_traj_t *ref,
                           const void *q, int64_t n) {
    if (!ctx) return bad_arg("null ctx");
    if (Refusal r = check_traj(traj, "traj", true)) return r;
    if (with_ref)
        if (Refusal r = check_traj(ref, "ref", true)) return r;
    if (!q) return bad_arg("%s: null query", name);
    if (n < 0) return bad_arg("negative n");
    return {};
}
inline Refusal series_span(const char *name, int64_t step_ns, int64_t capacity) {
    if (step_ns <= 0) return bad_arg("%s: step_ns must be > 0 (TimeSeries with a positive step)", name);
    if (capacity < 1 || capacity > INT32_MAX) return bad_arg("%s: capacity must be 1 .. 2^31 - 1", name);
    return {};
}
inline Refusal series_outputs(const char *name, const double *values, const int32_t *len) {
    if (!values || !len) return bad_arg("%s: values and len arrays required", name);
    return {};
}
// 1 .. `most` parameters of the enum `type_name`; `needs` is report_param_needs / gt_param_needs, *need the union of what they ask for
template <typename Query, typename Needs>
inline Refusal series_params(const char *name, const Query &q, int most, Needs needs, const char *type_name, int32_t *need) {
    if (q.n_params < 1 || q.n_params > most) return bad_arg("%s: n_params = %d, 1 .. %d parameters per call", name, q.n_params, most);
    for (int p = 0; p < q.n_params; ++p) {
        const int32_t k = needs(q.param[p]);
        if (k < 0) return bad_arg("%s: param[%d] = %d is not a %s", name, p, q.param[p], type_name);
        *need |= k;
    }
    return {};
}

inline Refusal check_values_series(const nyx_hip_ctx *ctx, const nyx_hip_traj_t *traj, int64_t n, const nyx_hip_values_query_t *q,
                                   int64_t capacity, const double *values, const int32_t *len) {
    const char *name = "traj_values";
    int32_t need = 0;
    if (Refusal r = series_open(name, ctx, traj, false, nullptr, q, n)) return r;
    if (Refusal r = series_params(name, *q, NYX_HIP_MAX_REPORT_PARAMS, report_param_needs, "nyx_hip_state_param", &need)) return r;
    if (Refusal r = series_span(name, q->step_ns, capacity)) return r;
    return series_outputs(name, values, len);
}

inline Refusal check_gt_series(const nyx_hip_ctx *ctx, const nyx_hip_traj_t *traj, int64_t n, const nyx_hip_gt_query_t *q,
                               int64_t capacity, const double *values, const int32_t *len) {
    const char *name = "traj_ground_track";
    int32_t need = 0;
    if (Refusal r = series_open(name, ctx, traj, false, nullptr, q, n)) return r;
    if (Refusal r = series_params(name, *q, NYX_HIP_MAX_GT_PARAMS, gt_param_needs, "nyx_hip_gt_param", &need)) return r;
    if (Refusal r = series_span(name, q->step_ns, capacity)) return r;
    if (q->frame.kind != NYX_HIP_ROT_IAU)
        return bad_arg("%s: frame.kind = %d, the frame must be an IAU-oriented frame (NYX_HIP_ROT_IAU)", name, q->frame.kind);
    if (q->frame.n_nut_prec < 0 || q->frame.n_nut_prec > NYX_HIP_MAX_NUT_PREC)
        return bad_arg("%s: frame.n_nut_prec = %d, 0 .. %d terms", name, q->frame.n_nut_prec, NYX_HIP_MAX_NUT_PREC);
    if ((need & GT_NEED_GEODETIC) && !(q->frame_eq_radius_km > 0.0)) return bad_arg("%s: Latitude / Height need frame_eq_radius_km > 0", name);
    if (!(q->frame_flattening >= 0.0 && q->frame_flattening < 1.0)) return bad_arg("%s: frame_flattening must be in [0, 1)", name);
    return series_outputs(name, values, len);
}

inline Refusal check_aer_series(const nyx_hip_ctx *ctx, const nyx_hip_traj_t *traj, int64_t n, const nyx_hip_aer_query_t *q,
                                int64_t capacity, const double *values, const int32_t *len) {
    const char *name = "traj_aer";
    int32_t need = 0;
    if (Refusal r = series_open(name, ctx, traj, false, nullptr, q, n)) return r;
    if (Refusal r = series_params(name, *q, NYX_HIP_MAX_AER_PARAMS, aer_param_needs, "nyx_hip_aer_param", &need)) return r;
    if (Refusal r = series_span(name, q->step_ns, capacity)) return r;
    if (q->n_stations < 1 || q->n_stations > NYX_HIP_MAX_STATIONS)
        return bad_arg("%s: n_stations = %d, 1 .. %d stations per call", name, q->n_stations, NYX_HIP_MAX_STATIONS);
    for (int s = 0; s < q->n_stations; ++s) {
        const nyx_hip_station_t &st = q->stations[s];
        if (!(st.latitude_deg >= -90.0 && st.latitude_deg <= 90.0)) return bad_arg("%s: stations[%d].latitude_deg must be in [-90, 90]", name, s);
        if (!std::isfinite(st.longitude_deg)) return bad_arg("%s: stations[%d].longitude_deg must be finite", name, s);
        if (!std::isfinite(st.height_km)) return bad_arg("%s: stations[%d].height_km must be finite", name, s);
        if (!(st.elevation_mask_deg >= -90.0 && st.elevation_mask_deg <= 90.0))
            return bad_arg("%s: stations[%d].elevation_mask_deg must be in [-90, 90]", name, s);
    }
    if (q->frame.kind != NYX_HIP_ROT_IAU)
        return bad_arg("%s: frame.kind = %d, the frame must be an IAU-oriented frame (NYX_HIP_ROT_IAU)", name, q->frame.kind);
    if (q->frame.n_nut_prec < 0 || q->frame.n_nut_prec > NYX_HIP_MAX_NUT_PREC)
        return bad_arg("%s: frame.n_nut_prec = %d, 0 .. %d terms", name, q->frame.n_nut_prec, NYX_HIP_MAX_NUT_PREC);
    if (!(q->frame_eq_radius_km > 0.0)) return bad_arg("%s: the stations stand on the ellipsoid, frame_eq_radius_km must be > 0", name);
    if (!(q->frame_flattening >= 0.0 && q->frame_flattening < 1.0)) return bad_arg("%s: frame_flattening must be in [0, 1)", name);
    return series_outputs(name, values, len);
}

// The eclipses are checked in two steps.  check_ecl_series is what its siblings are - it never dereferences the context - and
// refuses everything that can be told from the query alone.  check_ecl_context is what the query asks OF the context, checked once the
// query itself is sound: every chain segment is one of the context's `n_seg` (DevCfg.n_seg), and the context was not built with an
// integration-frame swap (`frame_swapped`: state_frame_body != 0) - the one refusal that is not a bad argument.  The chain rules
// themselves are chain_args.h's.
inline const char *ecl_body_name(char (&who)[32], const char *which, int index) {
    if (index < 0) std::snprintf(who, sizeof who, "%s", which);
    else std::snprintf(who, sizeof who, "%s[%d]", which, index);
    return who;
}
inline Refusal check_ecl_body(const char *name, const char *which, int index, const nyx_hip_ecl_body_t &b, int min_chain) {
    char who[32];
    ecl_body_name(who, which, index);
    if (Refusal r = check_chain(name, who, chain_view(b), min_chain)) return r;
    if (!(std::isfinite(b.mean_radius_km) && b.mean_radius_km > 0.0)) return bad_arg("%s: %s.mean_radius_km must be finite and > 0", name, who);
    return {};
}
inline Refusal check_ecl_series(const nyx_hip_ctx *ctx, const nyx_hip_traj_t *traj, int64_t n, const nyx_hip_ecl_query_t *q, int64_t capacity,
                                const double *values, const int32_t *len) {
    const char *name = "traj_eclipse";
    int32_t need = 0;
    if (Refusal r = series_open(name, ctx, traj, false, nullptr, q, n)) return r;
    if (Refusal r = series_params(name, *q, NYX_HIP_MAX_ECL_PARAMS, ecl_param_needs, "nyx_hip_ecl_param", &need)) return r;
    if (Refusal r = series_span(name, q->step_ns, capacity)) return r;
    if (q->n_bodies < 1 || q->n_bodies > NYX_HIP_MAX_ECL_BODIES)
        return bad_arg("%s: n_bodies = %d, 1 .. %d shadow bodies per call", name, q->n_bodies, NYX_HIP_MAX_ECL_BODIES);
    if (Refusal r = check_ecl_body(name, "light", -1, q->light, 1)) return r;
    for (int b = 0; b < q->n_bodies; ++b)
        if (Refusal r = check_ecl_body(name, "bodies", b, q->bodies[b], 0)) return r;
    for (int p = 0; p < q->n_params; ++p)
        if (ecl_param_per_body(q->param[p]) && (q->param_body[p] < 0 || q->param_body[p] >= q->n_bodies))
            return bad_arg("%s: param_body[%d] = %d, param[%d] is a per-body parameter of bodies[0 .. %d]", name, p, q->param_body[p], p, q->n_bodies - 1);
    return series_outputs(name, values, len);
}
// (of a query check_ecl_series has accepted)
inline Refusal check_ecl_context(const nyx_hip_ecl_query_t &q, int n_seg, bool frame_swapped) {
    const char *name = "traj_eclipse";
    for (int b = -1; b < q.n_bodies; ++b) {
        char who[32];
        ecl_body_name(who, b < 0 ? "light" : "bodies", b);
        if (Refusal r = check_chain_context(name, who, chain_view(b < 0 ? q.light : q.bodies[b]), n_seg)) return r;
    }
    if (frame_swapped)   // NYX_HIP_RC_UNSUPPORTED
        return frame_swap_refusal(name, "the first stored state of its trajectories is in another frame than the rest, an eclipse series of them is not defined");
    return {};
}

// The encounter report (include/nyx_hip_frame.h): the pattern of the eclipses with ONE chain, the target's.  check_frame_series never
// dereferences the context; check_frame_context is what the query asks of it, for the reason check_ecl_context gives.
inline Refusal check_frame_series(const nyx_hip_ctx *ctx, const nyx_hip_traj_t *traj, int64_t n, const nyx_hip_frame_query_t *q, int64_t capacity,
                                  const double *values, const int32_t *len) {
    const char *name = "traj_frame_values";
    int32_t need = 0;
    if (Refusal r = series_open(name, ctx, traj, false, nullptr, q, n)) return r;
    if (Refusal r = series_params(name, *q, NYX_HIP_MAX_FRAME_PARAMS, frm_param_needs, "nyx_hip_frame_param", &need)) return r;
    if (Refusal r = series_span(name, q->step_ns, capacity)) return r;
    if (Refusal r = check_chain(name, "", chain_view(*q), 0)) return r;
    if (!(std::isfinite(q->mu_km3_s2) && q->mu_km3_s2 > 0.0)) return bad_arg("%s: mu_km3_s2 must be finite and > 0", name);
    return series_outputs(name, values, len);
}
// (of a query check_frame_series has accepted)
inline Refusal check_frame_context(const nyx_hip_frame_query_t &q, int n_seg, bool frame_swapped) {
    const char *name = "traj_frame_values";
    if (Refusal r = check_chain_context(name, "", chain_view(q), n_seg)) return r;
    if (frame_swapped)   // NYX_HIP_RC_UNSUPPORTED
        return frame_swap_refusal(name, "the first stored state of its trajectories is in another frame than the rest, a series of them about another centre is not defined");
    return {};
}

// (epoch0_ns and moments are optional)
inline Refusal check_ric_series(const nyx_hip_ctx *ctx, const nyx_hip_traj_t *traj, int64_t n, const nyx_hip_traj_t *ref, int64_t n_ref,
                                const nyx_hip_ric_query_t *q, int64_t capacity, const double *values, const int32_t *len) {
    const char *name = "traj_ric_diff";
    if (Refusal r = series_open(name, ctx, traj, true, ref, q, n)) return r;
    if (n_ref != 1 && n_ref != n)
        return bad_arg("%s: n_ref = %lld, one reference trajectory or one per run (n = %lld)", name, (long long)n_ref, (long long)n);
    if (Refusal r = series_span(name, q->step_ns, capacity)) return r;
    if (q->frame_of != 0 && q->frame_of != 1) return bad_arg("%s: frame_of = %d, 0 (run) or 1 (reference)", name, q->frame_of);
    if (q->transport != 0 && q->transport != 1) return bad_arg("%s: transport = %d, 0 or 1", name, q->transport);
    if (q->smooth_window < 0 || q->smooth_window > NYX_HIP_RIC_MAX_WINDOW || (q->smooth_window != 0 && q->smooth_window % 2 == 0))
        return bad_arg("%s: smooth_window = %d, 0 or an odd window up to %d", name, q->smooth_window, NYX_HIP_RIC_MAX_WINDOW);
    return series_outputs(name, values, len);
}

// The link report (include/nyx_hip_link.h): the opening of the RIC report (two trajectories, n_ref = 1 or n), then the pattern of the
// eclipses without a light source: the bodies may be none.  check_link_series never dereferences the context; check_link_context is
// what the query asks of it, for the reason check_ecl_context gives.  (epoch0_ns is optional)
inline Refusal check_link_series(const nyx_hip_ctx *ctx, const nyx_hip_traj_t *traj, int64_t n, const nyx_hip_traj_t *ref, int64_t n_ref,
                                 const nyx_hip_link_query_t *q, int64_t capacity, const double *values, const int32_t *len) {
    const char *name = "traj_link";
    int32_t need = 0;
    if (Refusal r = series_open(name, ctx, traj, true, ref, q, n)) return r;
    if (n_ref != 1 && n_ref != n)
        return bad_arg("%s: n_ref = %lld, one transmitter trajectory or one per run (n = %lld)", name, (long long)n_ref, (long long)n);
    if (Refusal r = series_params(name, *q, NYX_HIP_MAX_LINK_PARAMS, lnk_param_needs, "nyx_hip_link_param", &need)) return r;
    if (Refusal r = series_span(name, q->step_ns, capacity)) return r;
    if (q->n_bodies < 0 || q->n_bodies > NYX_HIP_MAX_LINK_BODIES)
        return bad_arg("%s: n_bodies = %d, 0 .. %d bodies per call", name, q->n_bodies, NYX_HIP_MAX_LINK_BODIES);
    for (int b = 0; b < q->n_bodies; ++b)
        if (Refusal r = check_ecl_body(name, "bodies", b, q->bodies[b], 0)) return r;
    for (int p = 0; p < q->n_params; ++p) {
        if (!lnk_param_per_body(q->param[p])) continue;
        if (q->n_bodies == 0) return bad_arg("%s: param[%d] is a per-body parameter and the query names no body (n_bodies = 0)", name, p);
        if (q->param_body[p] < 0 || q->param_body[p] >= q->n_bodies)
            return bad_arg("%s: param_body[%d] = %d, param[%d] is a per-body parameter of bodies[0 .. %d]", name, p, q->param_body[p], p, q->n_bodies - 1);
    }
    return series_outputs(name, values, len);
}
// (of a query check_link_series has accepted)
inline Refusal check_link_context(const nyx_hip_link_query_t &q, int n_seg, bool frame_swapped) {
    const char *name = "traj_link";
    for (int b = 0; b < q.n_bodies; ++b) {
        char who[32];
        ecl_body_name(who, "bodies", b);
        if (Refusal r = check_chain_context(name, who, chain_view(q.bodies[b]), n_seg)) return r;
    }
    if (frame_swapped)   // NYX_HIP_RC_UNSUPPORTED
        return frame_swap_refusal(name, "the first stored state of its trajectories is in another frame than the rest, a link series of them is not defined");
    return {};
}

// ---- the one output block of a report's host flavour: values[n_params][capacity][n] (station views: one row per station and
// parameter), then the optional moments [capacity][NYX_HIP_RIC_MOMENTS] and first epochs [n], then len[n] (Block<N>, dev_block.h)
enum { SB_VALUES, SB_MOMENTS, SB_EPOCH0, SB_LEN, SB_PARTS };
inline Block<SB_PARTS> series_block(int64_t n_params, int64_t capacity, int64_t n, bool moments, bool epoch0) {
    return Block<SB_PARTS>({(size_t)n_params * (size_t)capacity * (size_t)n * sizeof(double), moments ? (size_t)capacity * NYX_HIP_RIC_MOMENTS * sizeof(double) : 0,
                            epoch0 ? (size_t)n * sizeof(int64_t) : 0, (size_t)n * sizeof(int32_t)});
}

// ---- a span of samples in chunks of consecutive samples, one per grid.y: sixteen a chunk, more where that would take more than
// kMaxChunks chunks
constexpr int64_t kChunkSamples = 16, kMaxChunks = 32768;
struct SeriesChunks { int64_t samples_per_block; unsigned grid_y; };
inline SeriesChunks series_chunks(int64_t span) {
    int64_t spb = kChunkSamples;
    if ((span + spb - 1) / spb > kMaxChunks) spb = (span + kMaxChunks - 1) / kMaxChunks;
    return {spb, (unsigned)((span + spb - 1) / spb)};
}
