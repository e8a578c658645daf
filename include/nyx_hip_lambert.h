/* nyx_hip_lambert.h — Lambert transfers on the device: a batch of independent problems, and a departure x arrival grid (a porkchop).
 *
 * What `tools/lambert::izzo` computes for one pair of states - the velocities of the conic that joins r1 to r2 in tof_s about a centre
 * of mu_km3_s2, with `LambertSolution::c3_km2_s2`, `v_inf_outgoing_declination_deg` and the rest on top - for n problems at once, or
 * for every cell of a grid of departure and arrival epochs whose body states come from the ephemerides OF THE CONTEXT.
 *
 *     nyx_hip_lambert_batch   values[p * n + i]                      status[i]                i < n
 *     nyx_hip_lambert_grid    values[(p * n_dep + i) * n_arr + j]    status[i * n_arr + j]    i < n_dep, j < n_arr
 *
 * The grid's block is a [rows = n_params, capacity = n_dep, n = n_arr] block as nyx_hip_series_stats (include/nyx_hip_stats.h) takes it.
 * Every value of a problem whose status is not NYX_HIP_LMB_OK is NaN.  Nothing else is written.
 *
 * THE DEFINITION (nyx_amd/lambert.py restates it on the host; csrc/lambert_dev.h is the device's text).  D. Izzo, "Revisiting
 * Lambert's problem" (2014), arranged as the reference's izzo.rs: one rounding per operation, sums of three as ((a0 + a1) + a2).
 *
 *     n1 = |r1|, n2 = |r2|, c = |r2 - r1|, s = ((n1 + n2) + c) * 0.5, i1 = r1 / n1, i2 = r2 / n2
 *     h = i1 x i2, ih = h / |h|                    the NATURAL normal, never flipped
 *     lam = sqrt(1 - c / s)
 *     SHORT: lambda = +lam, t_k = ih x i_k;  LONG: lambda = -lam, t_k = i_k x ih;  both tangents renormalised
 *     AUTO:  dnu = atan2(r2.y, r2.x) - atan2(r1.y, r1.x), + 2 pi if negative; LONG where dnu > pi (prograde about +z), else SHORT
 *     T = sqrt(2 mu / s^3) * tof_s
 *     find_xy, initial_guess, compute_t_min and halley (with T frozen at its first value), householder (with the 1e-14 denominators),
 *     the stop test |p - p0| < tol |p0| + tol, and reconstruct: as izzo.rs writes them, with n_revs and high_path being the
 *     `m` and `!low_path` arguments of its find_xy.
 *
 * FOUR DEPARTURES FROM THE REFERENCE.
 * 1. The normal.  The reference flips ih to +z where (r1 x r2).z < 0 and neither negates lambda nor reverses the tangents, which
 *    lamberthub (the code it was adapted from) does.  For r1 = (8000, 0, 0) km, r2 = (0, -8000, 0) km, 3600 s, mu = 398600.433 its
 *    ShortWay, LongWay and Auto each deliver a velocity that, flown, arrives 16 000 km from r2 (the same for r2 = (0, -7000, -500));
 *    with the natural normal all arrive within 3.2e-7 km.  Where (r1 x r2).z > 0 the rule above is the reference operation for
 *    operation; where it is < 0 it is lamberthub's.
 * 2. The series window.  The series of the time equation is used for m == 0 && x > 0 && 0.6 < x x < 1.4, the closed form everywhere
 *    else.  The reference tests x x alone: for negative x the argument of hyp2f1b reaches 1.4 (+inf from 1 on; just below 1 tens of
 *    thousands of terms, 59 447 measured; never ending on a NaN).  For x > 0 the argument is within 0.4 in magnitude and at most 43
 *    terms are needed (measured over an 801 x 401 grid of lambda and x).  hyp2f1b stops when the sum no longer changes or after
 *    NYX_HIP_LMB_SERIES_MAX = 64 terms.
 * 3. The way applies to multi-revolution requests too (the reference's public entry pins them to the prograde way and the low path).
 * 4. The closed form of the time equation without its cancellations.  As written in the reference, psi = acos(x y + lambda (1 - x x)) and
 *    T = ((psi + m pi) / sqrt|1 - x x| - x + lambda y) / (1 - x x): as lambda -> +-1, psi -> 0 and half an ulp of the acos argument is
 *    1.1e-16 / sin(psi) in psi, and x - lambda y cancels.  Measured on an Earth -> Moon grid about the Sun (lambda = 0.97, psi = 0.025): that
 *    form moves its own root by 3.2e-13, 53 times K eps (|T / T'| + |x|), when the start of its last step moves by two ulp.  Here
 *    psi = atan2(eta sqrt(1 - x x), x y + lambda (1 - x x)) on an ellipse, asinh(eta sqrt(x x - 1)) on a hyperbola, and where lambda x > 0
 *    eta = y - lambda x = (1 - lambda^2) / (y + lambda x),  x - lambda y = (1 - lambda^2)(x^2 (1 + lambda^2) - lambda^2) / (x + lambda y);
 *    elsewhere the differences as written.  The same experiment then moves the root by 0.1 of that bound.  T is the same function.
 * Kept as written: Halley's iteration in compute_t_min never updates T (lamberthub and poliastro do the same); it only moves the
 * feasibility edge of a multi-revolution request.
 *
 * Every loop is bounded on both sides: max_iter (1 .. 1000, the reference's 1000) for Halley and Householder, 64 terms for the series.
 *
 * THE PARAMETERS, with w = v_init - v_body1 (the reference's sign conventions: its v_inf_outgoing is v_body1 - v_init, negated again
 * for the declination and the right ascension):
 *     TRANSFER_ANGLE_DEG = acos(clip(i1 . i2)) in degrees for SHORT, 360 minus that for LONG, either plus 360 n_revs
 *     C3 = (w.x^2 + w.y^2) + w.z^2,  VINF_DEP = sqrt(C3),  DLA_DEG = asin(w.z / VINF_DEP),  RLA_DEG = atan2(w.y, w.x)
 *     VINF_ARR = |v_body2 - v_final|,  DV_TOTAL = VINF_DEP + VINF_ARR
 *
 * THE GRID.  Departure i is at dep0_ns + i * dep_step_ns.  Arrival j is at arr0_ns + j * arr_step_ns (has_tof = 0), or at the
 * departure's epoch plus tof0_ns + j * tof_step_ns (has_tof = 1).  Epochs become seconds as everywhere in this library
 * (csrc/hifitime_dev.h), tof_s is formed from the INTEGER nanosecond difference.  A body's state about the centre is
 * chain(body) - chain(centre), component by component, each chain the signed sum of its segments in chain order from zero
 * (include/nyx_hip_frame.h: the same Clenshaw recurrence with its companion derivative); n_chain = 0 is the context's integration
 * centre.  A cell with an epoch outside a segment of one of its chains is NYX_HIP_LMB_EPHEM_RANGE (this wins over the rest), a cell
 * whose arrival is not after its departure NYX_HIP_LMB_BAD_INPUT.
 *
 * This header is separate from nyx_hip.h on purpose: NYX_HIP_ABI_VERSION and the declaration list of nyx_hip.h (from which the Rust
 * `sys.rs` block is generated) are unchanged by it.
 */
#ifndef NYX_HIP_LAMBERT_H
#define NYX_HIP_LAMBERT_H

#include "nyx_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NYX_HIP_LAMBERT_VERSION 1
#define NYX_HIP_MAX_LAMBERT_PARAMS 8
#define NYX_HIP_LMB_SERIES_MAX 64
#define NYX_HIP_LMB_MAX_REVS 255
#define NYX_HIP_LMB_MAX_ITER 1000
#define NYX_HIP_LMB_TOL_MIN 1e-13
#define NYX_HIP_LMB_TOL_MAX 1e-2

/* Values are part of the ABI: never renumber. */
enum nyx_hip_lambert_way { NYX_HIP_LMB_AUTO = 0, NYX_HIP_LMB_SHORT = 1, NYX_HIP_LMB_LONG = 2, NYX_HIP_LMB_WAY_COUNT = 3 };

enum nyx_hip_lambert_status {
    NYX_HIP_LMB_OK = 0,
    NYX_HIP_LMB_BAD_INPUT = 1,    /* a non-finite component, n1 == 0, n2 == 0 or tof_s <= 0 */
    NYX_HIP_LMB_DEGENERATE = 2,   /* c == 0 (the reference's assert |ll| < 1), or |h| == 0 (plane undefined at 0 or pi) */
    NYX_HIP_LMB_NOT_FEASIBLE = 3, /* n_revs > m_max */
    NYX_HIP_LMB_TOO_CLOSE = 4,    /* a denominator below 1e-14 in Halley or Householder */
    NYX_HIP_LMB_MAX_ITER_HIT = 5, /* iteration limit reached */
    NYX_HIP_LMB_EPHEM_RANGE = 6   /* grid only: an epoch outside a chain's segments */
};

enum nyx_hip_lambert_param {
    NYX_HIP_LMB_V1X = 0, NYX_HIP_LMB_V1Y = 1, NYX_HIP_LMB_V1Z = 2,   /* km/s, v_init */
    NYX_HIP_LMB_V2X = 3, NYX_HIP_LMB_V2Y = 4, NYX_HIP_LMB_V2Z = 5,   /* km/s, v_final */
    NYX_HIP_LMB_X = 6,                   /* Izzo's variable */
    NYX_HIP_LMB_ITERATIONS = 7,          /* Householder steps taken, as a double */
    NYX_HIP_LMB_TOF_S = 8,
    NYX_HIP_LMB_TRANSFER_ANGLE_DEG = 9,
    NYX_HIP_LMB_C3 = 10,                 /* km^2/s^2 */
    NYX_HIP_LMB_VINF_DEP = 11,           /* km/s */
    NYX_HIP_LMB_DLA_DEG = 12,
    NYX_HIP_LMB_RLA_DEG = 13,
    NYX_HIP_LMB_VINF_ARR = 14,           /* km/s */
    NYX_HIP_LMB_DV_TOTAL = 15,           /* km/s */
    NYX_HIP_LMB_COUNT = 16
};

/* The solver's settings, shared by both entries */
typedef struct nyx_hip_lambert_query {
    int32_t n_params;                           /* 1 .. NYX_HIP_MAX_LAMBERT_PARAMS */
    int32_t param[NYX_HIP_MAX_LAMBERT_PARAMS];  /* enum nyx_hip_lambert_param; the first n_params are read */
    int32_t way;                                /* enum nyx_hip_lambert_way */
    int32_t n_revs;                             /* 0 .. 255 complete revolutions */
    int32_t high_path;                          /* 0: the low path (the reference's), 1: the other solution of a multi-revolution request */
    int32_t max_iter;                           /* 1 .. 1000 */
    int32_t _pad;
    double tol;                                 /* atol and rtol of the stop test; 1e-13 .. 1e-2 (the reference: 1e-4) */
} nyx_hip_lambert_query_t;

typedef struct nyx_hip_lambert_chain {
    int32_t n_chain;                           /* 0 = the integration centre itself */
    int32_t chain_segment[NYX_HIP_MAX_CHAIN];  /* indices into the context's segments */
    int32_t chain_sign[NYX_HIP_MAX_CHAIN];     /* +1 / -1 */
    int32_t _pad;
} nyx_hip_lambert_chain_t;

typedef struct nyx_hip_lambert_grid_query {
    nyx_hip_lambert_query_t solve;
    nyx_hip_lambert_chain_t dep, arr, centre;  /* the departure body, the arrival body, the transfer's centre */
    int32_t has_tof, _pad;                     /* 0: arrivals by epoch (arr0_ns, arr_step_ns), 1: by time of flight (tof0_ns, tof_step_ns) */
    int64_t n_dep, n_arr;                      /* >= 0; a grid without cells launches nothing */
    int64_t dep0_ns, dep_step_ns;              /* dep_step_ns > 0 */
    int64_t arr0_ns, arr_step_ns;              /* arr_step_ns > 0 (read when !has_tof) */
    int64_t tof0_ns, tof_step_ns;              /* tof_step_ns > 0 (read when has_tof) */
    double mu_km3_s2;                          /* of the centre; finite, > 0 */
} nyx_hip_lambert_grid_query_t;

/* n independent problems on host arrays.  rv1 / rv2 are the departure and arrival bodies' FULL states, component-major:
 * rv[c * n + i], c = 0 .. 5 (km, km/s); tof_s[i] in seconds.  n = 0 is legal and launches nothing.  Returns NYX_HIP_RC_BAD_ARG (and a
 * nyx_hip_last_error text) for, in this order: a null context or query, n_params outside 1..8, an unknown parameter, an unknown way,
 * n_revs outside 0..255, high_path not 0 / 1, tol outside [1e-13, 1e-2], max_iter outside 1..1000, mu_km3_s2 not finite and > 0,
 * n < 0, a NULL array.  Nothing is launched then. */
int32_t nyx_hip_lambert_batch(nyx_hip_ctx *ctx, const double *rv1, const double *rv2, const double *tof_s, int64_t n, double mu_km3_s2,
                              const nyx_hip_lambert_query_t *q, double *values, int32_t *status);

/* Device pointers, asynchronous on `hip_stream` (a hipStream_t; NULL = the default stream), ordered after the context's earlier
 * launches like the other *_device entries. */
int32_t nyx_hip_lambert_batch_device(nyx_hip_ctx *ctx, const double *rv1, const double *rv2, const double *tof_s, int64_t n, double mu_km3_s2,
                                     const nyx_hip_lambert_query_t *q, double *values, int32_t *status, void *hip_stream);

/* The porkchop: n_params * n_dep * n_arr doubles and n_dep * n_arr status words come back.  Refused like the batch (the solver's
 * settings first), then: n_dep or n_arr < 0 or more than 2^31 - 1 cells a side, dep_step_ns <= 0, the arrival's step <= 0, has_tof not
 * 0 / 1, a NULL array, a chain longer than 4, a segment index that is not one of the context's, a sign that is not +1 / -1, a
 * departure or arrival chain EQUAL to the centre's (the radius would be zero by construction); NYX_HIP_RC_UNSUPPORTED for a context
 * with an integration-frame swap (as the encounter report). */
int32_t nyx_hip_lambert_grid(nyx_hip_ctx *ctx, const nyx_hip_lambert_grid_query_t *q, double *values, int32_t *status);

int32_t nyx_hip_lambert_grid_device(nyx_hip_ctx *ctx, const nyx_hip_lambert_grid_query_t *q, double *values, int32_t *status, void *hip_stream);

/* Layout check for mirrors: 0 = sizeof(nyx_hip_lambert_query_t), 1 = NYX_HIP_LAMBERT_VERSION, 2 = NYX_HIP_LMB_COUNT,
 * 3 = NYX_HIP_MAX_LAMBERT_PARAMS, 4 = sizeof(nyx_hip_lambert_grid_query_t), 5 = sizeof(nyx_hip_lambert_chain_t); anything else -1. */
int32_t nyx_hip_lambert_sizeof(int32_t which);

#ifdef __cplusplus
}
#endif
#endif /* NYX_HIP_LAMBERT_H */
