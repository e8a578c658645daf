/* nyx_hip_eclipse.h — eclipses on the device: how much of the light source every run of an ensemble sees, over time.
 *
 * What `ShadowModel::compute` (cosmic/eclipse.rs:69-83) computes for one state - the apparent disk of the light source, the
 * apparent disk of every shadow body, the share of the first disk that the second hides, the body with the largest share - for
 * every trajectory an ensemble left on the device and every sample.  `nyx_hip_traj_eclipse` resamples like
 * nyx_hip_traj_ground_track (include/nyx_hip_groundtrack.h, whose contract this header follows word for word), evaluates the
 * ephemerides OF THE CONTEXT at the sample's epoch, and writes only the values:
 *
 *     values[(p * capacity + k) * n + i]   value of param[p] of sample k of trajectory i
 *     len[i]                               samples PRODUCED for trajectory i (those beyond `capacity` are counted, not stored)
 *
 * Sample k of trajectory i is taken at lo_i + k * step_ns, with lo_i = the smallest stored epoch of the trajectory and
 * hi_i = the largest (has_window = 0), or lo_i = max(start_ns, first epoch), hi_i = min(end_ns, last epoch)
 * (has_window = 1).  The series has (hi_i - lo_i) / step_ns + 1 samples, none when hi_i < lo_i or the trajectory is
 * empty; it ends at the first sample that cannot be interpolated (traj_it.rs:39-61), which `len[i]` then names.  Every
 * stored slot k >= len[i] (k < capacity) holds NaN: the caller never has to clear `values`.  Nothing is written beyond
 * n_params * capacity * n doubles.
 *
 * THE DEFINITION (anise's `Almanac::solar_eclipsing` as the propagator of this library restates it: `occultation_pct`).  The
 * position of a body (the light source included) w.r.t. the context's integration centre is the signed sum of the CONTEXT's
 * ephemeris segments along its chain, in chain order, every segment by the SPK type 2 Clenshaw recurrence.  With r the
 * interpolated inertial position, R_s / R_b the mean radii of the light source and of the body,
 *
 *     r_eb = r - p_body,  r_ls = p_sun - r                                      (no aberration, no light time)
 *     ls_p = R_s >= |r_ls| ? R_s : asin(R_s / |r_ls|)                           apparent radius of the light source
 *     fo_p = R_b >= |r_eb| ? R_b : asin(R_b / |r_eb|)                           apparent radius of the body
 *     d_p  = acos(-(r_ls . r_eb) / (|r_eb| |r_ls|))                             separation of the two centres
 *     d_p - ls_p > fo_p                      0                                  lit
 *     fo_p > d_p + ls_p                      100                                umbra
 *     |ls_p - fo_p| < d_p < ls_p + fo_p      100 (A(fo_p, d1) + A(ls_p, d2)) / (pi ls_p^2)      penumbra (100 where that is NaN)
 *         d1 = (d_p^2 - ls_p^2 + fo_p^2) / (2 d_p),  d2 = (d_p^2 + ls_p^2 - fo_p^2) / (2 d_p),  A(r, d) = r^2 acos(d / r) - d sqrt(r^2 - d^2)
 *     otherwise                              100 fo_p^2 / ls_p^2                annular
 *
 * THE QUIRK IS KEPT: an apparent radius whose body is nearer than its own radius is taken as the radius in km; for such a sample
 * the degree-valued parameters report what the percentage formula used (that number times 180 / pi).  The shadow model's
 * percentage is the largest over the bodies, strict >, first wins (`ShadowModel::compute`).
 *
 * TWO RULES OF THIS REPORT'S OWN.  A sample whose epoch lies outside a segment of a chain in use (NYX_HIP_ERR_EPHEM_RANGE of
 * the Clenshaw evaluation) ENDS THE SERIES exactly like a sample that cannot be interpolated: `len[i]` names it, NaN follows.
 * A context built with state_frame_body != 0 (integration-frame swap) is refused with NYX_HIP_RC_UNSUPPORTED: the first stored
 * state of its trajectories is in another frame than the rest.
 *
 * This header is separate from nyx_hip.h on purpose: NYX_HIP_ABI_VERSION and the declaration list of nyx_hip.h (from
 * which the Rust `sys.rs` block is generated) are unchanged by it.
 */
#ifndef NYX_HIP_ECLIPSE_H
#define NYX_HIP_ECLIPSE_H

#include "nyx_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NYX_HIP_ECL_VERSION 1
#define NYX_HIP_MAX_ECL_PARAMS 8
#define NYX_HIP_MAX_ECL_BODIES 8

/* Values are part of the ABI: never renumber. */
enum nyx_hip_ecl_param {
    /* of the whole shadow model (ShadowModel::compute: the body with the largest percentage, strict >, first wins) */
    NYX_HIP_ECL_OCCULTATION = 0,          /* percent, 0 .. 100 */
    NYX_HIP_ECL_ILLUMINATION = 1,         /* |percentage / 100 - 1|, the k of SolarPressure::eom */
    NYX_HIP_ECL_STATE = 2,                /* 0 lit (pct == 0), 1 partial (0 < pct < 100, annular included), 2 umbra (pct == 100) */
    NYX_HIP_ECL_ECLIPSING_BODY = 3,       /* index into query.bodies of the winner, -1 when the percentage is 0 */
    NYX_HIP_ECL_SUN_RANGE = 4,            /* km, |r_ls| */
    NYX_HIP_ECL_SUN_APPARENT_RADIUS = 5,  /* deg, ls_p */
    /* of ONE body, query.param_body[p] */
    NYX_HIP_ECL_BODY_OCCULTATION = 6,     /* percent */
    NYX_HIP_ECL_BODY_APPARENT_RADIUS = 7, /* deg, fo_p */
    NYX_HIP_ECL_BODY_SEPARATION = 8,      /* deg, d_p: Sun centre to body centre as seen from the spacecraft */
    NYX_HIP_ECL_BODY_PENUMBRA_MARGIN = 9, /* deg, d_p - ls_p - fo_p: > 0 fully lit; its zero is the penumbra edge */
    NYX_HIP_ECL_BODY_UMBRA_MARGIN = 10,   /* deg, fo_p - d_p - ls_p: > 0 in the umbra */
    NYX_HIP_ECL_COUNT = 11
};

/* A body by its position w.r.t. the context's integration centre = signed sum of the CONTEXT's segments (config.segments) */
typedef struct nyx_hip_ecl_body {
    int32_t n_chain;                          /* 0 = the integration centre itself */
    int32_t chain_segment[NYX_HIP_MAX_CHAIN]; /* indices into the context's segments */
    int32_t chain_sign[NYX_HIP_MAX_CHAIN];    /* +1 / -1 */
    int32_t _pad;
    double mean_radius_km;                    /* finite, > 0 */
} nyx_hip_ecl_body_t;

typedef struct nyx_hip_ecl_query {
    int32_t n_params;                             /* 1 .. NYX_HIP_MAX_ECL_PARAMS */
    int32_t param[NYX_HIP_MAX_ECL_PARAMS];        /* enum nyx_hip_ecl_param; the first n_params are read */
    int32_t param_body[NYX_HIP_MAX_ECL_PARAMS];   /* index into `bodies`; read for params >= NYX_HIP_ECL_BODY_OCCULTATION only */
    int32_t has_window;                           /* 0: every(step); 1: every_between(step, start, end) */
    int64_t step_ns;                              /* > 0 */
    int64_t start_ns, end_ns;                     /* read when has_window */
    nyx_hip_ecl_body_t light;                     /* the light source: n_chain 1 .. NYX_HIP_MAX_CHAIN */
    int32_t n_bodies;                             /* 1 .. NYX_HIP_MAX_ECL_BODIES */
    int32_t _pad;
    nyx_hip_ecl_body_t bodies[NYX_HIP_MAX_ECL_BODIES]; /* the shadow bodies, the first n_bodies are read */
} nyx_hip_ecl_query_t;

/* Host arrays: `traj` is staged on the device as nyx_hip_traj_every stages it; n_params * capacity * n doubles and n lengths
 * come back.  Returns NYX_HIP_RC_BAD_ARG (and a nyx_hip_last_error text) for n_params outside 1..8, an unknown parameter,
 * step_ns <= 0, capacity < 1, n < 0, a NULL array, n_bodies outside 1..8, a body or the light source with n_chain outside 0..4
 * (light: 1..4), a segment index that is not one of the context's, a sign that is not +1 / -1 or a radius that is not finite
 * and > 0, param_body outside 0 .. n_bodies - 1 for a per-body parameter; NYX_HIP_RC_UNSUPPORTED for a context with an
 * integration-frame swap; nothing is launched then. */
int32_t nyx_hip_traj_eclipse(nyx_hip_ctx *ctx, const nyx_hip_traj_t *traj, int64_t n, const nyx_hip_ecl_query_t *q, int64_t capacity,
                             double *values, int32_t *len);

/* Device pointers (traj's arrays, values, len), asynchronous on `hip_stream` (a hipStream_t; NULL = the default stream),
 * ordered after the context's earlier launches like the other *_device entries. */
int32_t nyx_hip_traj_eclipse_device(nyx_hip_ctx *ctx, const nyx_hip_traj_t *traj, int64_t n, const nyx_hip_ecl_query_t *q,
                                    int64_t capacity, double *values, int32_t *len, void *hip_stream);

/* Layout check for mirrors: 0 = sizeof(nyx_hip_ecl_query_t), 1 = NYX_HIP_ECL_VERSION, 2 = NYX_HIP_ECL_COUNT,
 * 3 = NYX_HIP_MAX_ECL_PARAMS, 4 = NYX_HIP_MAX_ECL_BODIES, 5 = sizeof(nyx_hip_ecl_body_t); anything else -1. */
int32_t nyx_hip_ecl_sizeof(int32_t which);

#ifdef __cplusplus
}
#endif
#endif /* NYX_HIP_ECLIPSE_H */
