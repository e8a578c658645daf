/* nyx_hip_link.h — the link report on the device: range, Doppler and line of sight from one spacecraft to every run of an ensemble.
 *
 * What `InterlinkTxSpacecraft::measure_instantaneous` (od/interlink/trk_device.rs) forms for a receiver trajectory seen from a
 * transmitter trajectory - the range, the Doppler, whether a body blocks the line between the two - for every trajectory an
 * ensemble left on the device and every sample.  `nyx_hip_traj_link` resamples BOTH trajectories like nyx_hip_traj_ric_diff
 * (include/nyx_hip_ric.h, whose span and series rules this header follows word for word), evaluates the ephemerides OF THE
 * CONTEXT at the sample's epoch like nyx_hip_traj_eclipse (include/nyx_hip_eclipse.h), and writes only the values:
 *
 *     values[(p * capacity + k) * n + i]   value of param[p] of sample k of run i
 *     len[i]                               samples PRODUCED for run i (those beyond `capacity` are counted, not stored)
 *     epoch0_ns[i]                         lo_i, the epoch of sample 0 (0 when the series is empty); may be NULL
 *
 * `traj` holds the receivers, the n runs.  `ref` holds the transmitter: n_ref = 1 trajectory (one for the whole ensemble) or
 * n_ref = n (pairwise).  Sample k of run i is taken at lo_i + k * step_ns, lo_i = max(first_i, first_ref[, start_ns]),
 * hi_i = min(last_i, last_ref[, end_ns]), first / last the smallest / largest stored epoch of a trajectory.  The series has
 * (hi_i - lo_i) / step_ns + 1 samples, none when hi_i < lo_i or either trajectory is empty, and ends at the first sample at which
 * EITHER trajectory cannot be interpolated, or whose epoch lies outside a segment of a chain in use (NYX_HIP_ERR_EPHEM_RANGE of
 * the Clenshaw evaluation, as the eclipse report), which `len[i]` then names.  Every stored slot k >= len[i] (k < capacity)
 * holds NaN.  Nothing is written beyond n_params * capacity * n doubles.
 *
 * THE DEFINITION (nyx_amd/links.py restates it operation for operation).  With r_rx, v_rx the interpolated state of the run,
 * r_tx, v_tx that of the transmitter, both in the inertial frame of the context's centre, rho = r_rx - r_tx, and sums of three
 * formed as ((a0 + a1) + a2):
 *
 *     Range            |rho|
 *     RangeRate        rho . (v_rx - v_tx) / |rho|                the physical one
 *     ReferenceDoppler rho . v_rx / |rho|                         what the reference forms AS WRITTEN: it transforms the receiver
 *                      into `observer.orbit.frame`, which is the common centre and not the transmitter, so the velocity there is
 *                      the receiver's own, despite the comment beside it ("velocity of the receiver w.r.t. the transmitter")
 *     RelativeSpeed    |v_rx - v_tx|
 *     LosX / Y / Z     rho / |rho|, transmitter to receiver, in the inertial frame
 *
 * OBSTRUCTION is Vallado's SIGHT test, which the reference's `almanac.line_of_sight_obstructed` call implements.  anise's source
 * is not part of the reference tree: this restates the published formula and is parity-unpinned, like the other anise
 * restatements of this project (nyx_hip_aer.h, nyx_hip_ric.h).  With b the position of the body - the signed sum of the CONTEXT's
 * segments along its chain, in chain order, at the sample's epoch; zero for an empty chain, the context's centre -,
 * r1 = r_rx - b, r2 = r_tx - b and R the body's mean radius:
 *
 *     r1sq = r1 . r1,  r2sq = r2 . r2,  d = r1 . r2
 *     tau  = (r1sq - d) / ((r1sq + r2sq) - 2 d)
 *     d2   = tau < 0 ? r1sq : (tau > 1 ? r2sq : (1 - tau) r1sq + d tau)
 *     obstructs = (tau >= 0 && tau <= 1 && d2 <= R R)
 *     BodyClearance = sqrt(d2) - R,  BodyObstructs = obstructs ? 1 : 0
 *
 * Visible is 1 when no body of `bodies` obstructs, else 0; ObstructingBody the index of the first that does, else -1; Clearance
 * the minimum over the bodies of BodyClearance (strict <, starting from +inf, first wins, a NaN never wins).  The reference
 * obstructs with the transmitter's orbit frame, that is the centre with its mean equatorial radius: bodies = {empty chain, that
 * radius}.  Further bodies are this library's extension.  With n_bodies = 0: Visible = 1, ObstructingBody = -1, Clearance = +inf.
 *
 * COINCIDENT SPACECRAFT (rho = 0) give a NaN tau: not obstructed, BodyClearance NaN (which Clearance, by its rule, passes over:
 * +inf when no other body gives a number), RangeRate / ReferenceDoppler / Los NaN.  Such a sample still counts in len[i].  Not
 * guarded.
 *
 * Every parameter uses only + - x /, sqrt and comparisons, all IEEE operations: compiled with -ffp-contract=off the device
 * agrees with the host definition to the last bit.  The two interpolated states are bit-identical to what nyx_hip_traj_every /
 * nyx_hip_traj_at return (the same device code).
 *
 * OUT OF SCOPE: light time, aberration, measurement noise, the integration-time average of `measure` (this is the instantaneous
 * geometry only) and antenna masks.  A context built with state_frame_body != 0 (integration-frame swap) is refused with
 * NYX_HIP_RC_UNSUPPORTED, as the eclipse report refuses it.
 *
 * Like its siblings this header leaves NYX_HIP_ABI_VERSION and the declaration list of nyx_hip.h unchanged.
 */
#ifndef NYX_HIP_LINK_H
#define NYX_HIP_LINK_H

#include "nyx_hip.h"
#include "nyx_hip_eclipse.h" /* nyx_hip_ecl_body_t: a chain into the context's segments plus a mean radius */

#ifdef __cplusplus
extern "C" {
#endif

#define NYX_HIP_LINK_VERSION 1
#define NYX_HIP_MAX_LINK_PARAMS 8
#define NYX_HIP_MAX_LINK_BODIES 8

/* Values are part of the ABI: never renumber. */
enum nyx_hip_link_param {
    NYX_HIP_LNK_RANGE = 0,             /* km, |rho| */
    NYX_HIP_LNK_RANGE_RATE = 1,        /* km/s, rho . (v_rx - v_tx) / |rho| */
    NYX_HIP_LNK_REFERENCE_DOPPLER = 2, /* km/s, rho . v_rx / |rho|: the reference's value as written */
    NYX_HIP_LNK_VISIBLE = 3,           /* 1 when no body obstructs, else 0 */
    NYX_HIP_LNK_OBSTRUCTING_BODY = 4,  /* index into query.bodies of the first body that obstructs, else -1 */
    NYX_HIP_LNK_CLEARANCE = 5,         /* km, the minimum over the bodies of BodyClearance; +inf without bodies */
    NYX_HIP_LNK_RELATIVE_SPEED = 6,    /* km/s, |v_rx - v_tx| */
    NYX_HIP_LNK_LOS_X = 7,             /* rho / |rho|, transmitter to receiver, inertial */
    NYX_HIP_LNK_LOS_Y = 8,
    NYX_HIP_LNK_LOS_Z = 9,
    /* of ONE body, query.param_body[p] */
    NYX_HIP_LNK_BODY_CLEARANCE = 10,   /* km, sqrt(d2) - R: the closest point of the segment to the body's centre, less its radius */
    NYX_HIP_LNK_BODY_OBSTRUCTS = 11,   /* 1 / 0 */
    NYX_HIP_LNK_COUNT = 12
};

typedef struct nyx_hip_link_query {
    int32_t n_params;                               /* 1 .. NYX_HIP_MAX_LINK_PARAMS */
    int32_t param[NYX_HIP_MAX_LINK_PARAMS];         /* enum nyx_hip_link_param; the first n_params are read */
    int32_t param_body[NYX_HIP_MAX_LINK_PARAMS];    /* index into `bodies`; read for params >= NYX_HIP_LNK_BODY_CLEARANCE only */
    int32_t has_window;                             /* 0: the whole overlap of run and transmitter; 1: clamped to [start_ns, end_ns] */
    int64_t step_ns;                                /* > 0 */
    int64_t start_ns, end_ns;                       /* read when has_window */
    int32_t n_bodies;                               /* 0 .. NYX_HIP_MAX_LINK_BODIES */
    int32_t _pad;
    nyx_hip_ecl_body_t bodies[NYX_HIP_MAX_LINK_BODIES]; /* the bodies that can block the line, the first n_bodies are read */
} nyx_hip_link_query_t;

/* Host arrays: `traj` and `ref` are staged on the device as nyx_hip_traj_ric_diff stages its inputs; n_params * capacity * n
 * doubles, n lengths and, when asked for, n first epochs come back.  Returns NYX_HIP_RC_BAD_ARG (and a nyx_hip_last_error text)
 * for a NULL required array, n < 0, n_ref not 1 or n, n_params outside 1..8, an unknown parameter, step_ns <= 0, capacity < 1,
 * n_bodies outside 0..8, a body with n_chain outside 0..4, a segment index that is not one of the context's, a sign that is not
 * +1 / -1 or a radius that is not finite and > 0, a per-body parameter with n_bodies = 0 or param_body outside
 * 0 .. n_bodies - 1; NYX_HIP_RC_UNSUPPORTED for a context with an integration-frame swap; nothing is launched then. */
int32_t nyx_hip_traj_link(nyx_hip_ctx *ctx, const nyx_hip_traj_t *traj, int64_t n, const nyx_hip_traj_t *ref, int64_t n_ref,
                          const nyx_hip_link_query_t *q, int64_t capacity, double *values, int32_t *len, int64_t *epoch0_ns);

/* Device pointers (the arrays of traj and ref, values, len, epoch0_ns), asynchronous on `hip_stream` (a hipStream_t; NULL = the
 * default stream), ordered after the context's earlier launches like the other *_device entries. */
int32_t nyx_hip_traj_link_device(nyx_hip_ctx *ctx, const nyx_hip_traj_t *traj, int64_t n, const nyx_hip_traj_t *ref, int64_t n_ref,
                                 const nyx_hip_link_query_t *q, int64_t capacity, double *values, int32_t *len, int64_t *epoch0_ns,
                                 void *hip_stream);

/* Layout check for mirrors: 0 = sizeof(nyx_hip_link_query_t), 1 = NYX_HIP_LINK_VERSION, 2 = NYX_HIP_LNK_COUNT,
 * 3 = NYX_HIP_MAX_LINK_PARAMS, 4 = NYX_HIP_MAX_LINK_BODIES; anything else -1. */
int32_t nyx_hip_link_sizeof(int32_t which);

#ifdef __cplusplus
}
#endif
#endif /* NYX_HIP_LINK_H */
