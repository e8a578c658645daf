/* nyx_hip_stats.h — ensemble statistics of a series report on the device: extremes, moments and exact quantiles over the runs.
 *
 * Every fused series report (nyx_hip_reports.h, _groundtrack.h, _aer.h, _eclipse.h, _frame.h, _link.h, _ric.h) leaves
 * values[rows][capacity][n] on the device, one row per parameter and one column per run.  A Monte Carlo consumer wants that
 * block reduced per sample: the 1 % / 50 % / 99 % band of a parameter over time, its mean and sigma, the worst run and which
 * one it was.  `nyx_hip_series_stats[_device]` is that reduction for ANY such block; `nyx_hip_traj_series_stats` runs a report
 * and the reducer back to back so that only the statistics cross the bus:
 *
 *     stats[((r * capacity) + k) * (NYX_HIP_STAT_FIXED + n_probs) + s]     column s of row r, sample k
 *
 * THE DEFINITION (nyx_amd/stats.py restates it).  For row r and sample k, with values[(r * capacity + k) * n + i] the value of
 * run i: H is the set of runs with status[i] == 0 (every run when `status` is NULL) and k < min(len[i], capacity); C the runs of
 * H whose value is not NaN; F the runs of C whose value is finite.  The fixed columns are enum nyx_hip_stat below; column
 * NYX_HIP_STAT_FIXED + j is the quantile prob[j] of C.
 *
 * The TOTAL ORDER is that of the IEEE bit pattern mapped to a monotone unsigned key: -inf < finite < +inf, -0.0 before +0.0.
 * MIN / MAX are the extremes of C in it, ARGMIN / ARGMAX the smallest run index that attains them (as a double; -1 for an
 * empty C).  SHIFT is the value of the smallest-index run of F (0.0 when F is empty), SUM the sum over F of d = v - SHIFT (one
 * rounded subtraction), SUMSQ that of d * d (each product rounded once); mean = SHIFT + SUM / FINITE and
 * var = (SUMSQ - SUM^2 / FINITE) / (FINITE - 1) are derived, the shift keeps them conditioned.
 *
 * A QUANTILE follows numpy's `linear` rule by a formula of this library, so that device and host round alike: s = C sorted in the
 * total order, m = |C|, h = (m - 1) * p, lo = floor(h), g = h - lo; the result is s[lo] when g == 0 or s[lo] == s[lo + 1], else
 * s[lo] + g * (s[lo + 1] - s[lo]).  So p = 0 gives MIN, p = 1 gives MAX, and two equal infinities never form inf - inf.  The
 * selection is EXACT at every n: a radix select on the 64-bit key, no sampling and no sketch.
 *
 * Every NaN this library writes into a column (MIN, MAX and the quantiles of an empty C; -inf beside a larger value under the
 * formula) is the one quiet NaN 0x7FF8000000000000.
 *
 * Integer columns and quantiles are exact; SUM and SUMSQ are added in an order that depends on n only (strided lanes, a
 * butterfly inside a wave, the waves in index order): the same call twice gives the same bits.
 *
 * n == 0 is not an error: every (r, k) then holds the empty pattern - HELD, COUNT, FINITE 0, the extremes and quantiles NaN,
 * the arguments -1, SHIFT, SUM, SUMSQ 0.  The caller never clears `stats`; nothing is written beyond
 * n_rows * capacity * (NYX_HIP_STAT_FIXED + n_probs) doubles.
 *
 * nyx_hip_last_kernel_ms after any of the three entries is the time of the REDUCER's launch alone; the report's own launch of
 * the fused entry is timed by calling that report by itself.
 *
 * OUT OF SCOPE: statistics across ranks (quantiles do not all-reduce; a sharded ensemble is reduced per rank or gathered
 * first), weighted runs, and RIC's own 28 sums, which stay with nyx_hip_traj_ric_diff.
 *
 * Like its siblings this header leaves NYX_HIP_ABI_VERSION and the declaration list of nyx_hip.h unchanged.
 */
#ifndef NYX_HIP_STATS_H
#define NYX_HIP_STATS_H

#include "nyx_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NYX_HIP_STATS_VERSION 1
#define NYX_HIP_STAT_FIXED 10
#define NYX_HIP_MAX_STAT_PROBS 8

/* Values are part of the ABI: never renumber. */
enum nyx_hip_stat {
    NYX_HIP_STAT_HELD = 0,    /* |H| */
    NYX_HIP_STAT_COUNT = 1,   /* |C| */
    NYX_HIP_STAT_MIN = 2,     /* over C in the total order; NaN when C is empty */
    NYX_HIP_STAT_MAX = 3,
    NYX_HIP_STAT_ARGMIN = 4,  /* the smallest run index that attains it, as a double; -1 when C is empty */
    NYX_HIP_STAT_ARGMAX = 5,
    NYX_HIP_STAT_FINITE = 6,  /* |F| */
    NYX_HIP_STAT_SHIFT = 7,   /* the value of the smallest-index run of F; 0.0 when F is empty */
    NYX_HIP_STAT_SUM = 8,     /* sum over F of d = v - SHIFT */
    NYX_HIP_STAT_SUMSQ = 9    /* sum over F of d * d */
    /* NYX_HIP_STAT_FIXED + j: the quantile prob[j] of C; NaN when C is empty */
};

typedef struct nyx_hip_stats_query {
    int32_t n_probs;                       /* 0 .. NYX_HIP_MAX_STAT_PROBS */
    int32_t reserved;                      /* 0 */
    double prob[NYX_HIP_MAX_STAT_PROBS];   /* each in [0, 1]; the first n_probs are read */
} nyx_hip_stats_query_t;

/* Values are part of the ABI: never renumber.  The report nyx_hip_traj_series_stats runs, and the type `query` points to. */
enum nyx_hip_series_kind {
    NYX_HIP_SERIES_VALUES = 0,        /* nyx_hip_values_query_t, rows = n_params */
    NYX_HIP_SERIES_GROUND_TRACK = 1,  /* nyx_hip_gt_query_t, rows = n_params */
    NYX_HIP_SERIES_AER = 2,           /* nyx_hip_aer_query_t, rows = n_stations * n_params */
    NYX_HIP_SERIES_ECLIPSE = 3,       /* nyx_hip_ecl_query_t, rows = n_params */
    NYX_HIP_SERIES_FRAME = 4,         /* nyx_hip_frame_query_t, rows = n_params */
    NYX_HIP_SERIES_LINK = 5,          /* nyx_hip_link_query_t, rows = n_params; needs `ref` */
    NYX_HIP_SERIES_RIC = 6,           /* nyx_hip_ric_query_t, rows = 6; needs `ref` */
    NYX_HIP_SERIES_COUNT = 7
};

/* Device pointers (values, len, status, stats), asynchronous on `hip_stream` (a hipStream_t; NULL = the default stream), ordered
 * after the context's earlier launches like the other *_device entries: it composes with the seven *_device reports and with
 * nyx_hip_propagate_batch_with_traj_device, nothing returns to the host in between.  `status` may be NULL.  Returns
 * NYX_HIP_RC_BAD_ARG (and a nyx_hip_last_error text) for a NULL ctx, q, values (n > 0), len (n > 0) or stats, n_probs outside
 * 0..8, a prob that is NaN or outside [0, 1], n_rows < 1, capacity outside 1 .. 2^31 - 1, n outside 0 .. 2^31 - 1; nothing is
 * launched then. */
int32_t nyx_hip_series_stats_device(nyx_hip_ctx *ctx, const double *values, const int32_t *len, const int32_t *status, int64_t n_rows,
                                    int64_t capacity, int64_t n, const nyx_hip_stats_query_t *q, double *stats, void *hip_stream);

/* Host arrays: values, len and status are staged on the device, reduced, and the statistics copied back.  For small callers and
 * tests; a report's block that is already on the device goes through the entry above. */
int32_t nyx_hip_series_stats(nyx_hip_ctx *ctx, const double *values, const int32_t *len, const int32_t *status, int64_t n_rows,
                             int64_t capacity, int64_t n, const nyx_hip_stats_query_t *q, double *stats);

/* The fused host entry: the trajectories are staged as the host flavour of report `kind` stages them, the report's *_device entry
 * writes its values into a device block, the reducer follows on the same stream, and only `stats`
 * [rows][capacity][NYX_HIP_STAT_FIXED + n_probs], `len` [n] and, for LINK and RIC when asked for, `epoch0_ns` [n] (else NULL) come
 * back.  `query` points to the query of that kind and `query_size` must be the library's sizeof of it (the guard of the void
 * pointer).  `status` [n] (host, may be NULL) leaves the runs with status != 0 out of the statistics, not out of the report.
 * Refused first, with NYX_HIP_RC_BAD_ARG and nothing launched: a NULL ctx, traj, query, sq, stats or len, an unknown kind, a
 * wrong query_size, a `ref` for a kind without one, no `ref` for LINK or RIC, the probabilities as above; then the refusals of
 * the report itself, with its own code and message. */
int32_t nyx_hip_traj_series_stats(nyx_hip_ctx *ctx, int32_t kind, const nyx_hip_traj_t *traj, int64_t n, const nyx_hip_traj_t *ref,
                                  int64_t n_ref, const void *query, int64_t query_size, int64_t capacity, const int32_t *status,
                                  const nyx_hip_stats_query_t *sq, double *stats, int32_t *len, int64_t *epoch0_ns);

/* Layout check for mirrors: 0 = sizeof(nyx_hip_stats_query_t), 1 = NYX_HIP_STATS_VERSION, 2 = NYX_HIP_STAT_FIXED,
 * 3 = NYX_HIP_MAX_STAT_PROBS, 4 = NYX_HIP_SERIES_COUNT; anything else -1. */
int32_t nyx_hip_stats_sizeof(int32_t which);

#ifdef __cplusplus
}
#endif
#endif /* NYX_HIP_STATS_H */
