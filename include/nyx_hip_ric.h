/* nyx_hip_ric.h — fused device report: RIC dispersions of an ensemble against a nominal.
 *
 * What a dispersion analysis reads from a Monte Carlo: the difference of every run to a nominal trajectory in the radial /
 * in-track / cross-track frame, over time, with the sums its mean and covariance envelope are made of.  The reference offers
 * the per-trajectory half as `Traj::ric_diff_to_parquet` (md/trajectory/traj.rs:407-600): align the two time spans, resample
 * both trajectories, `Orbit::ric_difference` of every pair, an in-place median filter over the result
 * (`smooth_state_diff_in_place`, md/trajectory/mod.rs:75-125).  `nyx_hip_traj_ric_diff` does that for a whole batch in one
 * pass on the device and writes only the six differences (and, when asked, 28 sums per sample):
 *
 *     values[(c * capacity + k) * n + i]   component c of sample k of run i: c = 0..2 dR, dI, dC (km), 3..5 dvR, dvI, dvC (km/s)
 *     len[i]                               samples PRODUCED for run i (those beyond `capacity` are counted, not stored)
 *     epoch0_ns[i]                         lo_i, the epoch of sample 0 (0 when the series is empty); may be NULL
 *     moments[k * 28 + q]                  may be NULL; q = 0 count, 1..6 sum d[c], 7..27 the row-major upper triangle of sum d d^T
 *
 * `ref` holds n_ref = 1 trajectory (one nominal for the whole ensemble) or n_ref = n (pairwise).  Sample k of run i is taken
 * at lo_i + k * step_ns, lo_i = max(first_i, first_ref[, start_ns]), hi_i = min(last_i, last_ref[, end_ns]), first / last
 * the smallest / largest stored epoch of a trajectory (a back-propagated batch works).  The series has
 * (hi_i - lo_i) / step_ns + 1 samples, none when hi_i < lo_i or either trajectory is empty, and ends at the first sample
 * at which EITHER trajectory cannot be interpolated (the reference zips two iterators that each stop at their first
 * failure), which `len[i]` then names.  Every stored slot k >= len[i] (k < capacity) holds NaN.  Nothing is written beyond
 * 6 * capacity * n doubles.
 *
 * The difference (definition: nyx_amd/params.py:ric_difference, restated operation for operation): d = run - ref,
 * differenced first; f = the run (frame_of = 0, the reference's `self.ric_difference(&other)`) or the reference trajectory
 * (frame_of = 1); r^ = f_r / |f_r|, h = f_r x f_v, c^ = h / |h|, i^ = c^ x r^; d_r and d_v projected on (r^, i^, c^); with
 * `transport`, w = |h| / (|f_r| |f_r|) and dv = (dv_R + w dr_I, dv_I - w dr_R, dv_C).  The transport term is the exact limit
 * of the finite-differenced DCM rate anise applies under two-body motion; anise's source is not part of the reference tree,
 * so this restates its documented definition and is parity-unpinned, like the other anise restatements of this project.
 * The two interpolated states are bit-identical to what nyx_hip_traj_every / nyx_hip_traj_at return (the same device code).
 *
 * smooth_window = 0 or 1: none; odd 3..9: the reference's in-place median filter with that window (it uses 5), applied to
 * the stored samples of a run (k < min(len[i], capacity)) when there are more of them than the window.
 *
 * The moments are taken after smoothing over the runs i with k < min(len[i], capacity), on a fixed grid in a fixed order and
 * without floating-point atomics: their bits depend on the inputs only.  They are indexed by SAMPLE: a time series of the
 * ensemble when all lo_i agree - the Monte Carlo case, every run and the nominal starting at one epoch.  A sharded host
 * adds the capacity * 28 doubles of its ranks with one all-reduce; mean = s / count, cov = (S - count m m^T) / (count - 1).
 *
 * Like nyx_hip_reports.h this header leaves NYX_HIP_ABI_VERSION and the declaration list of nyx_hip.h unchanged.
 */
#ifndef NYX_HIP_RIC_H
#define NYX_HIP_RIC_H

#include "nyx_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NYX_HIP_RIC_VERSION 1
#define NYX_HIP_RIC_MOMENTS 28      /* doubles per sample: count, 6 sums, 21 second moments */
#define NYX_HIP_RIC_MAX_WINDOW 9

typedef struct nyx_hip_ric_query {
    int64_t step_ns;            /* > 0 */
    int64_t start_ns, end_ns;   /* read when has_window */
    int32_t has_window;         /* 0: the whole overlap of run and reference; 1: clamped to [start_ns, end_ns] */
    int32_t frame_of;           /* 0: the frame of the run; 1: the frame of the reference trajectory */
    int32_t transport;          /* 0 / 1: remove the rotation of the frame from the velocity difference */
    int32_t smooth_window;      /* 0 or 1: none; odd 3 .. NYX_HIP_RIC_MAX_WINDOW */
} nyx_hip_ric_query_t;

/* Host arrays: `traj` and `ref` are staged on the device as nyx_hip_traj_values stages its input; 6 * capacity * n doubles,
 * n lengths and, when asked for, n first epochs and capacity * 28 moments come back.  Returns NYX_HIP_RC_BAD_ARG (and a
 * nyx_hip_last_error text) for step_ns <= 0, capacity < 1, n < 0, n_ref not 1 or n, frame_of or transport outside 0 / 1, an
 * even smooth_window or one above 9, or a NULL required array; nothing is launched then. */
int32_t nyx_hip_traj_ric_diff(nyx_hip_ctx *ctx, const nyx_hip_traj_t *traj, int64_t n, const nyx_hip_traj_t *ref, int64_t n_ref,
                              const nyx_hip_ric_query_t *q, int64_t capacity, double *values, int32_t *len, int64_t *epoch0_ns,
                              double *moments);

/* Device pointers (the arrays of traj and ref, values, len, epoch0_ns, moments), asynchronous on `hip_stream` (a hipStream_t;
 * NULL = the default stream), ordered after the context's earlier launches like the other *_device entries. */
int32_t nyx_hip_traj_ric_diff_device(nyx_hip_ctx *ctx, const nyx_hip_traj_t *traj, int64_t n, const nyx_hip_traj_t *ref, int64_t n_ref,
                                     const nyx_hip_ric_query_t *q, int64_t capacity, double *values, int32_t *len, int64_t *epoch0_ns,
                                     double *moments, void *hip_stream);

/* Layout check for mirrors: 0 = sizeof(nyx_hip_ric_query_t), 1 = NYX_HIP_RIC_VERSION, 2 = NYX_HIP_RIC_MOMENTS,
 * 3 = NYX_HIP_RIC_MAX_WINDOW; anything else -1. */
int32_t nyx_hip_ric_sizeof(int32_t which);

#ifdef __cplusplus
}
#endif
#endif /* NYX_HIP_RIC_H */
