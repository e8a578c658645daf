// stats_host.h - the host side of the statistics entries (include/nyx_hip_stats.h; host only, no HIP; abi.cpp,
// tests/cxx/stats_host_check.cpp): what they refuse before anything is launched, as data in the style of series_host.h, the rows and
// the query size of every kind of report, and the one device block of the host flavours (a Block<N>, dev_block.h).
#pragma once
#include "dev_block.h"
#include "series_host.h"
#include "stats_args.h"

inline Refusal check_stats_query(const char *name, const nyx_hip_stats_query_t *q) {
    if (!q) return bad_arg("%s: null statistics query", name);
    if (q->n_probs < 0 || q->n_probs > NYX_HIP_MAX_STAT_PROBS)
        return bad_arg("%s: n_probs = %d, 0 .. %d probabilities per call", name, q->n_probs, NYX_HIP_MAX_STAT_PROBS);
    for (int j = 0; j < q->n_probs; ++j)
        if (!(q->prob[j] >= 0.0 && q->prob[j] <= 1.0)) return bad_arg("%s: prob[%d] must lie in [0, 1]", name, j);   // (a NaN fails both)
    return {};
}

// nyx_hip_series_stats[_device]: a block of values (values and len may be null when there is no run)
inline Refusal check_series_stats(const nyx_hip_ctx *ctx, const double *values, const int32_t *len, int64_t n_rows, int64_t capacity, int64_t n,
                                  const nyx_hip_stats_query_t *q, const double *stats) {
    const char *name = "series_stats";
    if (!ctx) return bad_arg("null ctx");
    if (Refusal r = check_stats_query(name, q)) return r;
    if (n_rows < 1) return bad_arg("%s: n_rows must be >= 1", name);
    if (capacity < 1 || capacity > INT32_MAX) return bad_arg("%s: capacity must be 1 .. 2^31 - 1", name);
    if (n < 0 || n > INT32_MAX) return bad_arg("%s: n must be 0 .. 2^31 - 1", name);
    if (!stats) return bad_arg("%s: stats array required", name);
    if (n > 0 && (!values || !len)) return bad_arg("%s: values and len arrays required", name);
    return {};
}

// what a kind of report is to the fused entry: the size of its query, whether it takes a second batch, the name of its entry
struct SeriesKind { int64_t query_size; bool with_ref; const char *name; };
inline bool series_kind(int32_t kind, SeriesKind *out) {
    switch (kind) {
    case NYX_HIP_SERIES_VALUES: *out = {(int64_t)sizeof(nyx_hip_values_query_t), false, "traj_values"}; return true;
    case NYX_HIP_SERIES_GROUND_TRACK: *out = {(int64_t)sizeof(nyx_hip_gt_query_t), false, "traj_ground_track"}; return true;
    case NYX_HIP_SERIES_AER: *out = {(int64_t)sizeof(nyx_hip_aer_query_t), false, "traj_aer"}; return true;
    case NYX_HIP_SERIES_ECLIPSE: *out = {(int64_t)sizeof(nyx_hip_ecl_query_t), false, "traj_eclipse"}; return true;
    case NYX_HIP_SERIES_FRAME: *out = {(int64_t)sizeof(nyx_hip_frame_query_t), false, "traj_frame_values"}; return true;
    case NYX_HIP_SERIES_LINK: *out = {(int64_t)sizeof(nyx_hip_link_query_t), true, "traj_link"}; return true;
    case NYX_HIP_SERIES_RIC: *out = {(int64_t)sizeof(nyx_hip_ric_query_t), true, "traj_ric_diff"}; return true;
    default: return false;
    }
}
// the rows of the values block of a query of `kind` (of a query its own check has accepted)
inline int64_t series_kind_rows(int32_t kind, const void *query) {
    switch (kind) {
    case NYX_HIP_SERIES_VALUES: return ((const nyx_hip_values_query_t *)query)->n_params;
    case NYX_HIP_SERIES_GROUND_TRACK: return ((const nyx_hip_gt_query_t *)query)->n_params;
    case NYX_HIP_SERIES_AER: return (int64_t)((const nyx_hip_aer_query_t *)query)->n_stations * ((const nyx_hip_aer_query_t *)query)->n_params;
    case NYX_HIP_SERIES_ECLIPSE: return ((const nyx_hip_ecl_query_t *)query)->n_params;
    case NYX_HIP_SERIES_FRAME: return ((const nyx_hip_frame_query_t *)query)->n_params;
    case NYX_HIP_SERIES_LINK: return ((const nyx_hip_link_query_t *)query)->n_params;
    default: return 6;   // NYX_HIP_SERIES_RIC
    }
}

// nyx_hip_traj_series_stats, what is refused before the report's own checks
inline Refusal check_traj_series_stats(const nyx_hip_ctx *ctx, int32_t kind, const nyx_hip_traj_t *traj, const nyx_hip_traj_t *ref,
                                       const void *query, int64_t query_size, const nyx_hip_stats_query_t *sq, const double *stats,
                                       const int32_t *len) {
    const char *name = "traj_series_stats";
    if (!ctx) return bad_arg("null ctx");
    SeriesKind kd;
    if (!series_kind(kind, &kd)) return bad_arg("%s: kind = %d is not a nyx_hip_series_kind", name, kind);
    if (!traj) return bad_arg("%s: null traj", name);
    if (!query) return bad_arg("%s: null query", name);
    if (query_size != kd.query_size)
        return bad_arg("%s: query_size = %lld, the query of %s is %lld bytes", name, (long long)query_size, kd.name, (long long)kd.query_size);
    if (kd.with_ref && !ref) return bad_arg("%s: %s needs a second batch (ref)", name, kd.name);
    if (!kd.with_ref && ref) return bad_arg("%s: %s takes no second batch (ref)", name, kd.name);
    if (Refusal r = check_stats_query(name, sq)) return r;
    if (!stats || !len) return bad_arg("%s: stats and len arrays required", name);
    return {};
}

// ---- the device block of the host flavour: values [n_rows][capacity][n], stats [n_rows][capacity][S], len [n], status [n] (absent: size 0)
enum { STB_VALUES, STB_STATS, STB_LEN, STB_STATUS, STB_PARTS };
inline Block<STB_PARTS> stats_block(int64_t n_rows, int64_t capacity, int64_t n, int n_probs, bool status) {
    const size_t cells = (size_t)n_rows * (size_t)capacity, words = (size_t)n * sizeof(int32_t);
    return Block<STB_PARTS>({cells * (size_t)n * sizeof(double), cells * (size_t)(NYX_HIP_STAT_FIXED + n_probs) * sizeof(double), words, status ? words : 0});
}
