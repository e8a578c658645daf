/* nyx_hip_aer.h — station views on the device: azimuth, elevation, range and range rate of a whole ensemble from ground stations.
 *
 * What `GroundStation::azimuth_elevation_of` / `TrackingDevice::measure_instantaneous` (od/ground_station/mod.rs:69-105,
 * od/ground_station/trk_device.rs:158-208) compute for one state - the station placed by geodetic latitude / longitude / height
 * in an IAU body-fixed frame, the spacecraft expressed in that frame, azimuth / elevation / range / range rate in the station's
 * south-east-zenith (SEZ) triad, the measurement kept when the elevation is above the mask - for every trajectory an ensemble
 * left on the device, every sample and up to NYX_HIP_MAX_STATIONS stations.  `nyx_hip_traj_aer` resamples like
 * nyx_hip_traj_ground_track (include/nyx_hip_groundtrack.h, whose contract this header follows word for word), expresses every
 * interpolated state in `frame` AT THE SAMPLE'S EPOCH - ONE interpolation and ONE rotation per sample serve all stations - and
 * writes only the values:
 *
 *     values[((s * n_params + p) * capacity + k) * n + i]   value of param[p] of sample k of trajectory i seen from station s
 *     len[i]                                                samples PRODUCED for trajectory i (those beyond `capacity` are counted,
 *                                                           not stored); shared by all stations
 *
 * Sample k of trajectory i is taken at lo_i + k * step_ns, with lo_i = the smallest stored epoch of the trajectory and
 * hi_i = the largest (has_window = 0), or lo_i = max(start_ns, first epoch), hi_i = min(end_ns, last epoch)
 * (has_window = 1).  The series has (hi_i - lo_i) / step_ns + 1 samples, none when hi_i < lo_i or the trajectory is
 * empty; it ends at the first sample that cannot be interpolated (traj_it.rs:39-61), which `len[i]` then names.  Every
 * stored slot k >= len[i] (k < capacity) holds NaN: the caller never has to clear `values`.  Nothing is written beyond
 * n_stations * n_params * capacity * n doubles.
 *
 * THE DEFINITION (a restatement: anise's `azimuth_elevation_range_sez` is not part of the reference tree, so this is not pinned
 * against it).  For a station (phi, lambda, h, mask) on the ellipsoid (a, f) of the frame, e^2 = f (2 - f):
 *
 *     C = a / sqrt(1 - e^2 sin^2 phi),  S = C (1 - e^2)                                  (`Orbit::try_latlongalt`)
 *     r_st = [(C + h) cos phi cos lambda, (C + h) cos phi sin lambda, (S + h) sin phi]   body-fixed
 *     S^ = [sin phi cos lambda, sin phi sin lambda, -cos phi]
 *     E^ = [-sin lambda, cos lambda, 0]
 *     Z^ = [cos phi cos lambda, cos phi sin lambda, sin phi]
 *
 * These station constants are computed on the host, once per call, with the C library; the kernel only reads them.  Per sample,
 * with yf the state in the body-fixed frame (velocity R v - w x (R r), the station being at rest in that frame):
 *
 *     rho = yf[0..3] - r_st;  rho_S = rho . S^,  rho_E = rho . E^,  rho_Z = rho . Z^     (sums of three, left to right)
 *     range = sqrt(rho_S^2 + rho_E^2 + rho_Z^2)
 *     elevation = asin(rho_Z / range)  [deg]
 *     azimuth = atan2(rho_E, -rho_S)   [deg, [0, 360), the wrap rule of NYX_HIP_GT_LONGITUDE]
 *     range_rate = (rho_x vf_x + rho_y vf_y + rho_z vf_z) / range
 *     elevation_above_mask = elevation - mask;  visible = elevation_above_mask >= 0 ? 1 : 0   (a NaN elevation is not visible)
 *
 * The frame is the one of the ground tracks: the drift of the pole itself is neglected, which enters the range rate with at most
 * the ground-track figure, 5e-8 km/s at the Earth's surface - three orders below the reference's Doppler noise of 5e-5 km/s.
 * No light-time correction, no terrain mask beyond the one constant elevation, no obstruction by another body.
 *
 * This header is separate from nyx_hip.h on purpose: NYX_HIP_ABI_VERSION and the declaration list of nyx_hip.h (from
 * which the Rust `sys.rs` block is generated) are unchanged by it.
 */
#ifndef NYX_HIP_AER_H
#define NYX_HIP_AER_H

#include "nyx_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NYX_HIP_AER_VERSION 1
#define NYX_HIP_MAX_AER_PARAMS 8
#define NYX_HIP_MAX_STATIONS 16

/* Values are part of the ABI: never renumber. */
enum nyx_hip_aer_param {
    NYX_HIP_AER_AZIMUTH = 0,              /* deg, [0, 360), from north through east */
    NYX_HIP_AER_ELEVATION = 1,            /* deg */
    NYX_HIP_AER_RANGE = 2,                /* km */
    NYX_HIP_AER_RANGE_RATE = 3,           /* km/s */
    NYX_HIP_AER_ELEVATION_ABOVE_MASK = 4, /* deg: elevation - the station's mask */
    NYX_HIP_AER_VISIBLE = 5,              /* 1.0 where elevation >= mask, else 0.0 */
    NYX_HIP_AER_RHO_S = 6,                /* km: the line of sight in the station's SEZ triad */
    NYX_HIP_AER_RHO_E = 7,
    NYX_HIP_AER_RHO_Z = 8,
    NYX_HIP_AER_COUNT = 9
};

typedef struct nyx_hip_station {
    double latitude_deg;       /* geodetic, [-90, 90] */
    double longitude_deg;
    double height_km;          /* above the ellipsoid */
    double elevation_mask_deg; /* [-90, 90] */
} nyx_hip_station_t;

typedef struct nyx_hip_aer_query {
    int32_t n_params;                      /* 1 .. NYX_HIP_MAX_AER_PARAMS */
    int32_t param[NYX_HIP_MAX_AER_PARAMS]; /* enum nyx_hip_aer_param; the first n_params are read */
    int32_t has_window;                    /* 0: every(step); 1: every_between(step, start, end) */
    int64_t step_ns;                       /* > 0 */
    int64_t start_ns, end_ns;              /* read when has_window */
    int32_t has_frame;                     /* 0: identity orientation, the stations are at rest in the inertial frame */
    int32_t _pad;
    double frame_eq_radius_km;             /* > 0: the stations stand on the ellipsoid */
    double frame_flattening;               /* [0, 1) */
    nyx_hip_rotation_t frame;              /* NYX_HIP_ROT_IAU orientations only (read when has_frame) */
    int32_t n_stations;                    /* 1 .. NYX_HIP_MAX_STATIONS */
    int32_t _pad2;
    nyx_hip_station_t stations[NYX_HIP_MAX_STATIONS]; /* the first n_stations are read */
} nyx_hip_aer_query_t;

/* Host arrays: `traj` is staged on the device as nyx_hip_traj_every stages it; n_stations * n_params * capacity * n doubles and
 * n lengths come back.  Returns NYX_HIP_RC_BAD_ARG (and a nyx_hip_last_error text) for n_params outside 1..8, an unknown
 * parameter, step_ns <= 0, capacity < 1, n < 0, a NULL array, n_stations outside 1..16, a station with a latitude or a mask
 * outside [-90, 90] or a non-finite longitude / height, frame.kind != NYX_HIP_ROT_IAU, n_nut_prec outside
 * 0..NYX_HIP_MAX_NUT_PREC, frame_eq_radius_km <= 0 or a flattening outside [0, 1); nothing is launched then. */
int32_t nyx_hip_traj_aer(nyx_hip_ctx *ctx, const nyx_hip_traj_t *traj, int64_t n, const nyx_hip_aer_query_t *q, int64_t capacity,
                         double *values, int32_t *len);

/* Device pointers (traj's arrays, values, len), asynchronous on `hip_stream` (a hipStream_t; NULL = the default stream),
 * ordered after the context's earlier launches like the other *_device entries. */
int32_t nyx_hip_traj_aer_device(nyx_hip_ctx *ctx, const nyx_hip_traj_t *traj, int64_t n, const nyx_hip_aer_query_t *q,
                                int64_t capacity, double *values, int32_t *len, void *hip_stream);

/* Layout check for mirrors: 0 = sizeof(nyx_hip_aer_query_t), 1 = NYX_HIP_AER_VERSION, 2 = NYX_HIP_AER_COUNT,
 * 3 = NYX_HIP_MAX_AER_PARAMS, 4 = NYX_HIP_MAX_STATIONS; anything else -1. */
int32_t nyx_hip_aer_sizeof(int32_t which);

#ifdef __cplusplus
}
#endif
#endif /* NYX_HIP_AER_H */
