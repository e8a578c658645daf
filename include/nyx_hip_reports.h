/* nyx_hip_reports.h — fused device reports: StateParameter series of a whole ensemble.
 *
 * What a Monte Carlo consumer asks of the trajectories an ensemble left on the device (`Results::every_value_of`,
 * `every_value_of_between`, reference mc/results.rs:86-160): the value of a few state parameters of every run, every
 * `step_ns`.  `nyx_hip_traj_values` resamples (`Traj::every` / `Traj::every_between`, md/trajectory/traj.rs:148-162),
 * evaluates up to NYX_HIP_MAX_REPORT_PARAMS parameters from the SAME interpolated state, and writes only the values:
 *
 *     values[(p * capacity + k) * n + i]   value of param[p] of sample k of trajectory i   (step-major, like nyx_hip_traj_t)
 *     len[i]                               samples PRODUCED for trajectory i (those beyond `capacity` are counted, not stored)
 *
 * Sample k of trajectory i is taken at lo_i + k * step_ns, with lo_i = the smallest stored epoch of the trajectory and
 * hi_i = the largest (has_window = 0), or lo_i = max(start_ns, first epoch), hi_i = min(end_ns, last epoch)
 * (has_window = 1).  The series has (hi_i - lo_i) / step_ns + 1 samples, none when hi_i < lo_i or the trajectory is
 * empty; it ends at the first sample that cannot be interpolated (traj_it.rs:39-61), which `len[i]` then names.  Every
 * stored slot k >= len[i] (k < capacity) holds NaN: the caller never has to clear `values`.  Nothing is written beyond
 * n_params * capacity * n doubles.
 *
 * The interpolated state is bit-identical to what nyx_hip_traj_every / nyx_hip_traj_at return for that epoch (the same
 * device code).  The parameter definitions are the ones of the Python mirror (nyx_amd/params.py: classical osculating
 * elements from the Cartesian state and mu, angles in degrees in [0, 360)); like the event scalars they restate anise's
 * documented definitions and are parity-unpinned against that absent crate.
 *
 * This header is separate from nyx_hip.h on purpose: NYX_HIP_ABI_VERSION and the declaration list of nyx_hip.h (from
 * which the Rust `sys.rs` block is generated) are unchanged by it.
 */
#ifndef NYX_HIP_REPORTS_H
#define NYX_HIP_REPORTS_H

#include "nyx_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NYX_HIP_REPORTS_VERSION 1
#define NYX_HIP_MAX_REPORT_PARAMS 8

/* The orbit-derived members of StateParameter (md/param.rs).  Values are part of the ABI: never renumber. */
enum nyx_hip_state_param {
    NYX_HIP_SP_X = 0,                 /* km */
    NYX_HIP_SP_Y = 1,
    NYX_HIP_SP_Z = 2,
    NYX_HIP_SP_VX = 3,                /* km/s */
    NYX_HIP_SP_VY = 4,
    NYX_HIP_SP_VZ = 5,
    NYX_HIP_SP_RMAG = 6,              /* km */
    NYX_HIP_SP_VMAG = 7,              /* km/s */
    NYX_HIP_SP_HMAG = 8,              /* km^2/s */
    NYX_HIP_SP_ENERGY = 9,            /* km^2/s^2 */
    NYX_HIP_SP_SEMI_MAJOR_AXIS = 10,  /* km */
    NYX_HIP_SP_ECCENTRICITY = 11,
    NYX_HIP_SP_INCLINATION = 12,      /* deg, [0, 180] */
    NYX_HIP_SP_RAAN = 13,             /* deg, [0, 360) */
    NYX_HIP_SP_AOP = 14,              /* deg, [0, 360) */
    NYX_HIP_SP_TRUE_ANOMALY = 15,     /* deg, [0, 360) */
    NYX_HIP_SP_PERIOD = 16,           /* s */
    NYX_HIP_SP_APOAPSIS_RADIUS = 17,  /* km */
    NYX_HIP_SP_PERIAPSIS_RADIUS = 18, /* km */
    NYX_HIP_SP_COUNT = 19
};

typedef struct nyx_hip_values_query {
    int32_t n_params;                         /* 1 .. NYX_HIP_MAX_REPORT_PARAMS */
    int32_t has_window;                       /* 0: every(step); 1: every_between(step, start, end) */
    int32_t param[NYX_HIP_MAX_REPORT_PARAMS]; /* enum nyx_hip_state_param; the first n_params are read */
    int64_t step_ns;                          /* > 0 */
    int64_t start_ns, end_ns;                 /* read when has_window */
    double mu_km3_s2;                         /* <= 0: the central body of the context */
} nyx_hip_values_query_t;

/* Host arrays: `traj` is staged on the device as nyx_hip_traj_every stages it; n_params * capacity * n doubles and n
 * lengths come back.  Returns NYX_HIP_RC_BAD_ARG (and a nyx_hip_last_error text) for n_params outside 1..8, an unknown
 * parameter, step_ns <= 0, capacity < 1, n < 0 or a NULL array; nothing is launched then. */
int32_t nyx_hip_traj_values(nyx_hip_ctx *ctx, const nyx_hip_traj_t *traj, int64_t n, const nyx_hip_values_query_t *q,
                            int64_t capacity, double *values, int32_t *len);

/* Device pointers (traj's arrays, values, len), asynchronous on `hip_stream` (a hipStream_t; NULL = the default stream),
 * ordered after the context's earlier launches like the other *_device entries. */
int32_t nyx_hip_traj_values_device(nyx_hip_ctx *ctx, const nyx_hip_traj_t *traj, int64_t n, const nyx_hip_values_query_t *q,
                                   int64_t capacity, double *values, int32_t *len, void *hip_stream);

/* Layout check for mirrors: 0 = sizeof(nyx_hip_values_query_t), 1 = NYX_HIP_REPORTS_VERSION, 2 = NYX_HIP_SP_COUNT,
 * 3 = NYX_HIP_MAX_REPORT_PARAMS; anything else -1. */
int32_t nyx_hip_reports_sizeof(int32_t which);

#ifdef __cplusplus
}
#endif
#endif /* NYX_HIP_REPORTS_H */
