/* nyx_hip_groundtrack.h — ground tracks on the device: geodetic latitude / longitude / height of a whole ensemble.
 *
 * What `Traj::to_groundtrack_parquet` (md/trajectory/sc_traj.rs:131-155) writes for one trajectory - the state expressed in a
 * body-fixed frame, one sample every `step_ns`, as geodetic latitude, longitude, height and |r| - for every trajectory an
 * ensemble left on the device.  `nyx_hip_traj_ground_track` resamples like nyx_hip_traj_values (include/nyx_hip_reports.h,
 * whose contract this header follows word for word), expresses every interpolated state in `frame` AT THE SAMPLE'S EPOCH and
 * writes only the values:
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
 * The inertial state is bit-identical to what nyx_hip_traj_every / nyx_hip_traj_at return for that epoch (the same device
 * code).  The frame is the one of the stop conditions (nyx_hip_event_t): an IAU-oriented body-fixed frame of the SAME centre,
 * DCM = R3(W) R1(90 - delta) R3(90 + alpha), velocity R v - w x (R r) with w = dW/dt about the pole (the drift of the pole
 * itself is neglected, as there); the geodetic pair is the classical iteration of the event scalars, so a ground-track Height
 * equals the NYX_HIP_EV_HEIGHT_KM scalar of the same state and frame.  The host definition is nyx_amd/groundtrack.py.
 *
 * The reference rotates the STORED states and interpolates in the rotating frame; here the inertial state is interpolated and
 * rotated at the sample epoch.  The two differ by interpolation error only - an error that is below a micrometre where the stored
 * steps are even, but reaches KILOMETRES in windows that hold states a few seconds apart (the step controller at a shadow
 * crossing) and in the last interval, in either order; the inertial one is the closer there ("Ground tracks").
 *
 * This header is separate from nyx_hip.h on purpose: NYX_HIP_ABI_VERSION and the declaration list of nyx_hip.h (from
 * which the Rust `sys.rs` block is generated) are unchanged by it.
 */
#ifndef NYX_HIP_GROUNDTRACK_H
#define NYX_HIP_GROUNDTRACK_H

#include "nyx_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NYX_HIP_GROUNDTRACK_VERSION 1
#define NYX_HIP_MAX_GT_PARAMS 8

/* All evaluated on the state expressed in the body-fixed frame.  Values are part of the ABI: never renumber. */
enum nyx_hip_gt_param {
    NYX_HIP_GT_LATITUDE = 0,    /* geodetic, deg */
    NYX_HIP_GT_LONGITUDE = 1,   /* deg, [0, 360): NYX_HIP_EV_LONGITUDE_DEG, but an angle that rounds to 360 itself is 0 */
    NYX_HIP_GT_HEIGHT = 2,      /* geodetic, km */
    NYX_HIP_GT_RMAG = 3,        /* km */
    NYX_HIP_GT_DECLINATION = 4, /* deg: asin(z / |r|) */
    NYX_HIP_GT_X = 5,           /* km */
    NYX_HIP_GT_Y = 6,
    NYX_HIP_GT_Z = 7,
    NYX_HIP_GT_VX = 8,          /* km/s, relative to the rotating frame */
    NYX_HIP_GT_VY = 9,
    NYX_HIP_GT_VZ = 10,
    NYX_HIP_GT_VMAG = 11,       /* km/s: the ground-relative speed */
    NYX_HIP_GT_COUNT = 12
};

typedef struct nyx_hip_gt_query {
    int32_t n_params;                     /* 1 .. NYX_HIP_MAX_GT_PARAMS */
    int32_t param[NYX_HIP_MAX_GT_PARAMS]; /* enum nyx_hip_gt_param; the first n_params are read */
    int32_t has_window;                   /* 0: every(step); 1: every_between(step, start, end) */
    int64_t step_ns;                      /* > 0 */
    int64_t start_ns, end_ns;             /* read when has_window */
    int32_t has_frame;                    /* 0: identity orientation, the values are taken on the inertial state */
    int32_t _pad;
    double frame_eq_radius_km;            /* > 0 for Latitude / Height */
    double frame_flattening;              /* [0, 1) */
    nyx_hip_rotation_t frame;             /* NYX_HIP_ROT_IAU orientations only (read when has_frame) */
} nyx_hip_gt_query_t;

/* Host arrays: `traj` is staged on the device as nyx_hip_traj_every stages it; n_params * capacity * n doubles and n
 * lengths come back.  Returns NYX_HIP_RC_BAD_ARG (and a nyx_hip_last_error text) for n_params outside 1..8, an unknown
 * parameter, step_ns <= 0, capacity < 1, n < 0, a NULL array, frame.kind != NYX_HIP_ROT_IAU, n_nut_prec outside
 * 0..NYX_HIP_MAX_NUT_PREC, a geodetic parameter with frame_eq_radius_km <= 0 or a flattening outside [0, 1); nothing is
 * launched then. */
int32_t nyx_hip_traj_ground_track(nyx_hip_ctx *ctx, const nyx_hip_traj_t *traj, int64_t n, const nyx_hip_gt_query_t *q,
                                  int64_t capacity, double *values, int32_t *len);

/* Device pointers (traj's arrays, values, len), asynchronous on `hip_stream` (a hipStream_t; NULL = the default stream),
 * ordered after the context's earlier launches like the other *_device entries. */
int32_t nyx_hip_traj_ground_track_device(nyx_hip_ctx *ctx, const nyx_hip_traj_t *traj, int64_t n, const nyx_hip_gt_query_t *q,
                                         int64_t capacity, double *values, int32_t *len, void *hip_stream);

/* Layout check for mirrors: 0 = sizeof(nyx_hip_gt_query_t), 1 = NYX_HIP_GROUNDTRACK_VERSION, 2 = NYX_HIP_GT_COUNT,
 * 3 = NYX_HIP_MAX_GT_PARAMS; anything else -1. */
int32_t nyx_hip_groundtrack_sizeof(int32_t which);

#ifdef __cplusplus
}
#endif
#endif /* NYX_HIP_GROUNDTRACK_H */
