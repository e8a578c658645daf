/* nyx_hip_frame.h — the encounter report on the device: an ensemble seen from another body, over time.
 *
 * What `Traj::to_frame` (md/trajectory/sc_traj.rs:88-129: `almanac.transform_to(state.orbit, new_frame, None)` for every state)
 * followed by a parameter evaluation computes for one trajectory - the state translated to another centre of the same
 * orientation, then the orbital elements ABOUT THAT CENTRE and the B-plane of the approach (cosmic/bplane.rs) - for every
 * trajectory an ensemble left on the device and every sample.  `nyx_hip_traj_frame_values` resamples like nyx_hip_traj_eclipse
 * (include/nyx_hip_eclipse.h, whose contract this header follows section for section), evaluates the ephemerides OF THE CONTEXT at
 * the sample's epoch, and writes only the values:
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
 * THE DEFINITION.  The state of the target centre w.r.t. the context's integration centre is the signed sum of the CONTEXT's
 * ephemeris segments along the target's chain, in chain order - r = r + sign * p, v = v + sign * pv - every segment by the SPK
 * type 2 Clenshaw recurrence with its companion derivative:
 *
 *     w0 = cf[j] + (two_t * w1 - w2),  d0 = (2 * w1 + two_t * d1) - d2     j = n_coef - 1 .. 1
 *     p  = cf[0] + (t * w0 - w1),      pv = ((w0 + t * d0) - d1) / radius  t = (et - mid) / radius, two_t = 2 t
 *
 * The translated state is rv' = rv - (r, v), component by component (no aberration, no light time: the reference passes None
 * too); n_chain = 0 is the integration centre itself and the identity.  Codes 0 .. 18 are enum nyx_hip_state_param
 * (include/nyx_hip_reports.h), evaluated from rv' exactly as nyx_hip_traj_values evaluates them, with mu_km3_s2 of the TARGET.
 * The others, with rmag, vmag, h = r x v, hmag, sma, evec, ecc as that entry forms them and sums of three as ((a0 + a1) + a2):
 *
 *     C3         = vmag * vmag - 2 * mu / rmag
 *     e^ = evec / ecc,  h^ = h / hmag,  n^ = h^ x e^,  f = sqrt(1 - (1 / ecc) * (1 / ecc))
 *     s  = e^ / ecc + f * n^,  s^ = s / |s|                                the incoming asymptote
 *     b  = |sma| * sqrt(ecc * ecc - 1)                                     the semi-minor axis of the hyperbola
 *     B  = b * (f * e^ - (1 / ecc) * n^)
 *     t  = s^ x (0, 0, 1),  t^ = t / |t|,  r^ = s^ x t^
 *     BdotT = B . t^,  BdotR = B . r^,  BAngle = atan2(BdotR, BdotT) in degrees, in (-180, 180]
 *     BMagnitude = sqrt(BdotT^2 + BdotR^2),  VInfinity = sqrt(C3)
 *
 * The reference's third B-plane parameter, the linearised time of flight (`BLTOF`), has NO code: in its formula B . s^ is zero
 * analytically (B lies in the plane normal to S) and what is left is rounding noise.
 *
 * TWO RULES OF THIS REPORT'S OWN.  Where ecc <= 1 the orbit about the target is not a hyperbola (`BPlane::new` returns
 * NotHyperbolic): BdotT, BdotR, BAngle, BMagnitude and VInfinity of that sample are NaN AND THE SERIES CONTINUES - the other
 * parameters of the sample are unaffected, `len[i]` does not move.  A sample whose epoch lies outside a segment of the target's
 * chain (NYX_HIP_ERR_EPHEM_RANGE of the Clenshaw evaluation) ENDS THE SERIES exactly like a sample that cannot be interpolated:
 * `len[i]` names it, NaN follows.  A context built with state_frame_body != 0 (integration-frame swap) is refused with
 * NYX_HIP_RC_UNSUPPORTED: the first stored state of its trajectories is in another frame than the rest.
 *
 * This header is separate from nyx_hip.h on purpose: NYX_HIP_ABI_VERSION and the declaration list of nyx_hip.h (from
 * which the Rust `sys.rs` block is generated) are unchanged by it.
 */
#ifndef NYX_HIP_FRAME_H
#define NYX_HIP_FRAME_H

#include "nyx_hip.h"
#include "nyx_hip_reports.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NYX_HIP_FRAME_VERSION 1
#define NYX_HIP_MAX_FRAME_PARAMS 8

/* Values are part of the ABI: never renumber.  0 .. 18 are enum nyx_hip_state_param (NYX_HIP_SP_X .. NYX_HIP_SP_PERIAPSIS_RADIUS),
 * of the translated state and the target's mu. */
enum nyx_hip_frame_param {
    NYX_HIP_FRM_C3 = 19,          /* km^2/s^2, vmag^2 - 2 mu / rmag */
    NYX_HIP_FRM_B_DOT_T = 20,     /* km */
    NYX_HIP_FRM_B_DOT_R = 21,     /* km */
    NYX_HIP_FRM_B_ANGLE = 22,     /* deg, atan2(BdotR, BdotT) in (-180, 180] */
    NYX_HIP_FRM_B_MAGNITUDE = 23, /* km, sqrt(BdotT^2 + BdotR^2) */
    NYX_HIP_FRM_V_INFINITY = 24,  /* km/s, sqrt(C3) */
    NYX_HIP_FRM_COUNT = 25
};

typedef struct nyx_hip_frame_query {
    int32_t n_params, has_window;              /* 1 .. NYX_HIP_MAX_FRAME_PARAMS; 0: every(step), 1: every_between(step, start, end) */
    int32_t param[NYX_HIP_MAX_FRAME_PARAMS];   /* enum nyx_hip_frame_param; the first n_params are read */
    int64_t step_ns, start_ns, end_ns;         /* step_ns > 0; start_ns / end_ns read when has_window */
    int32_t n_chain;                           /* 0 = the integration centre itself */
    int32_t chain_segment[NYX_HIP_MAX_CHAIN];  /* indices into the context's segments */
    int32_t chain_sign[NYX_HIP_MAX_CHAIN];     /* +1 / -1 */
    int32_t _pad;
    double mu_km3_s2;                          /* of the target centre; finite, > 0 */
} nyx_hip_frame_query_t;

/* Host arrays: `traj` is staged on the device as nyx_hip_traj_every stages it; n_params * capacity * n doubles and n lengths
 * come back.  Returns NYX_HIP_RC_BAD_ARG (and a nyx_hip_last_error text) for n_params outside 1..8, an unknown parameter,
 * step_ns <= 0, capacity < 1, n < 0, a NULL array, n_chain outside 0..4, a segment index that is not one of the context's, a sign
 * that is not +1 / -1, mu_km3_s2 not finite and > 0; NYX_HIP_RC_UNSUPPORTED for a context with an integration-frame swap;
 * nothing is launched then. */
int32_t nyx_hip_traj_frame_values(nyx_hip_ctx *ctx, const nyx_hip_traj_t *traj, int64_t n, const nyx_hip_frame_query_t *q, int64_t capacity,
                                  double *values, int32_t *len);

/* Device pointers (traj's arrays, values, len), asynchronous on `hip_stream` (a hipStream_t; NULL = the default stream),
 * ordered after the context's earlier launches like the other *_device entries. */
int32_t nyx_hip_traj_frame_values_device(nyx_hip_ctx *ctx, const nyx_hip_traj_t *traj, int64_t n, const nyx_hip_frame_query_t *q,
                                         int64_t capacity, double *values, int32_t *len, void *hip_stream);

/* Layout check for mirrors: 0 = sizeof(nyx_hip_frame_query_t), 1 = NYX_HIP_FRAME_VERSION, 2 = NYX_HIP_FRM_COUNT,
 * 3 = NYX_HIP_MAX_FRAME_PARAMS; anything else -1. */
int32_t nyx_hip_frame_sizeof(int32_t which);

#ifdef __cplusplus
}
#endif
#endif /* NYX_HIP_FRAME_H */
