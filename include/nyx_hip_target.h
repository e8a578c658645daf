/* nyx_hip_target.h — the differential-correction targeter on the device: one Newton-Raphson loop per run of an ensemble.
 *
 * What `Targeter::try_achieve_fd` (md/opti/targeter.rs with raphson_finite_diff.rs, the branch without a finite burn) computes for
 * one spacecraft - the correction of chosen components of the state at a correction epoch that brings chosen parameters of the
 * propagated state to desired values at an achievement epoch - for every run of a batch at once.  A run needs 1 + V propagations per
 * iteration (the nominal and one per variable); all (1 + V) n of them are ONE launch of the context's propagator, and one kernel
 * evaluates the objectives and takes the Newton step of every run.  Nothing but a 4-byte counter crosses the bus per iteration.
 *
 * THE DEFINITION (nyx_amd/targeter.py restates it on the host; csrc/target_dev.h is the device's text; one rounding per operation,
 * every sum taken left to right from its first term).
 *
 *   start-up    xi_start = the run's state propagated to correction_epoch_ns
 *               c6 = 0; c6[component_j] += init_guess_j in the order of the variables; xi = apply(xi_start, c6)
 *               total_j = init_guess_j, prev = +inf
 *   apply       inertial: x[k] = x[k] + c6[k].  VNC: v[k] = v[k] + ((e0[k] c6[3] + e1[k] c6[4]) + e2[k] c6[5]) with e0 = v / |v|,
 *               e1 = (r x v) / |r x v|, e2 = e0 x e1 OF xi_start (csrc/predict_kernel.hip forms the same frame): ONE frame per run
 *   iteration it = 0 .. iterations
 *               the 1 + V states xi and apply(xi, perturbation_j e_component_j) are propagated to achievement_epoch_ns
 *               each final state is translated to the objective target (n_chain > 0: minus the signed sum of the chain's segments
 *               at the achievement epoch, include/nyx_hip_frame.h) and val_k[i] = the parameter obj_param[i] of it (mu_km3_s2)
 *               err_i = obj_mult[i] (obj_desired[i] - val_0[i]) + obj_add[i],   J[i][j] = (val_j[i] - val_0[i]) / perturbation_j
 *               every |err_i| <= obj_tolerance[i]: CONVERGED, iterations = it
 *               nrm = sqrt(sum err_i^2); | nrm - prev | < 1e-10: INEFFECTIVE; prev = nrm
 *               the solve (below); the clamp, one chain per variable, ON THE STEP, not on the total, as the reference writes it:
 *                   |d_j| > |max_step_j| -> |max_step_j| sign(d_j),  else d_j > max_value_j -> max_value_j,  else d_j < min_value_j -> min_value_j
 *               c6 from d as above, xi = apply(xi, c6), total_j += d_j
 *               it == iterations: TOO_MANY_ITERATIONS (after the step, as the reference falls out of its loop)
 *   a run that ends keeps its last total (`correction`), err (`achieved_errors`), nominal final state (`achieved`, about the
 *   context's centre) and `corrected` = apply(xi_start, c6 of total) (targeter.rs:538-563).
 *
 * TWO DEPARTURES FROM THE REFERENCE.
 * 1. The solve.  The reference forms a pseudo-inverse through nalgebra's `try_inverse` (an LU with
 * pivoting).  Here, with O objectives and V variables,
 *     O <  V:   (J J^T) y = err, d = J^T y        the minimum-norm step
 *     O >= V:   (J^T J) d = J^T err               the least-squares step
 * by an UNPIVOTED CHOLESKY factorisation written out operation for operation (L[i][j] = (G[i][j] - sum_{k<j} L[i][k] L[j][k]) / L[j][j],
 * L[i][i] = sqrt(..), forward and back substitution).  It is the same step; the Gram matrix is symmetric positive definite whenever
 * the pseudo-inverse exists, so no pivoting is needed - hence no dynamically indexed registers on the device - and no explicit inverse
 * is formed.  A pivot that is not finite or not > 0 gives SINGULAR.
 * 2. The VNC frame is that of xi_start for the whole run.  The reference applies the guess, every perturbation and every step in the
 *    frame of the CURRENT xi, sums the steps component by component, and reports corrected_state = xi_start with that sum applied in
 *    the frame of xi_start.  The frame turns with the velocity: for Eccentricity -> 0.4 and SemiMajorAxis -> 8100 km on the 8000 km,
 *    e = 0.2 orbit of its tests (a 3 km/s correction) the loop converges with its own xi in 17 iterations, and the reported
 *    correction, flown again, misses the eccentricity by 0.0723 (tolerance 1e-5).  With one frame the total IS the sum of the steps and
 *    `corrected` the state they led to (to rounding): the same case converges in 17 iterations, |dv| = 3.07203 km/s (3.08873 summed
 *    over turning frames), and holds when flown again.  In the inertial frame nothing differs from the reference.
 *
 * STATUS (which test wins is this order): EPHEM_RANGE (the achievement epoch lies outside a segment of the objective target's chain:
 * every run, at iteration 0), PROP_FAILED (one of the run's 1 + V rows, or its leg to the correction epoch, ended with a non-zero
 * propagation status), NOT_FINITE (an achieved value or a Jacobian entry is NaN or +-inf - a B-plane objective on an ellipse, the
 * reference's NotHyperbolic), CONVERGED, INEFFECTIVE, SINGULAR, TOO_MANY_ITERATIONS.
 *
 * THE LOOP runs on the host, under the context's lock for its whole length: one launch to the correction epoch, the seed kernel, then
 * per iteration one in-place propagation launch of the (1 + V) n work rows, the step kernel and a 4-byte read of the number of runs
 * still active; it ends when that is 0 or after iterations + 1 rounds (`iterations_run` rounds were run).  Runs that have ended ride
 * along with zero duration.  The device flavour therefore WAITS ON ITS STREAM ONCE PER ITERATION: it is not asynchronous and not
 * graph-capturable.  The work rows belong to the context and grow on demand.
 *
 * This header is separate from nyx_hip.h on purpose: NYX_HIP_ABI_VERSION and the declaration list of nyx_hip.h (from which the Rust
 * `sys.rs` block is generated) are unchanged by it.
 */
#ifndef NYX_HIP_TARGET_H
#define NYX_HIP_TARGET_H

#include "nyx_hip.h"
#include "nyx_hip_frame.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NYX_HIP_TARGET_VERSION 1
#define NYX_HIP_MAX_TARGET_VARS 6
#define NYX_HIP_MAX_TARGET_OBJS 6
#define NYX_HIP_TARGET_MAX_ITERATIONS 1000

/* Values are part of the ABI: never renumber. */
enum nyx_hip_target_status {
    NYX_HIP_TGT_OK_CONVERGED = 0,
    NYX_HIP_TGT_TOO_MANY_ITERATIONS = 1,
    NYX_HIP_TGT_INEFFECTIVE = 2,
    NYX_HIP_TGT_SINGULAR = 3,
    NYX_HIP_TGT_NOT_FINITE = 4,
    NYX_HIP_TGT_PROP_FAILED = 5,
    NYX_HIP_TGT_EPHEM_RANGE = 6,
    NYX_HIP_TGT_STATUS_COUNT = 7
};

/* The reference's `Vary`, the impulsive components only: the index of the state component */
enum nyx_hip_target_vary {
    NYX_HIP_VARY_POSITION_X = 0, NYX_HIP_VARY_POSITION_Y = 1, NYX_HIP_VARY_POSITION_Z = 2,
    NYX_HIP_VARY_VELOCITY_X = 3, NYX_HIP_VARY_VELOCITY_Y = 4, NYX_HIP_VARY_VELOCITY_Z = 5,
    NYX_HIP_VARY_COUNT = 6
};

typedef struct nyx_hip_target_query {
    int32_t n_vars, n_objs;                              /* 1 .. 6 each */
    int32_t iterations;                                  /* 0 .. 1000 (the reference: 100) */
    int32_t correction_frame;                            /* NYX_HIP_FRAME_INERTIAL (0) or NYX_HIP_FRAME_VNC (2) */
    int32_t var_component[NYX_HIP_MAX_TARGET_VARS];      /* enum nyx_hip_target_vary */
    double var_perturbation[NYX_HIP_MAX_TARGET_VARS];    /* finite, != 0 (the reference: 1e-4) */
    double var_init_guess[NYX_HIP_MAX_TARGET_VARS];
    double var_max_step[NYX_HIP_MAX_TARGET_VARS];        /* >= 0 (0.2) */
    double var_max_value[NYX_HIP_MAX_TARGET_VARS];       /* >= 0 (5) */
    double var_min_value[NYX_HIP_MAX_TARGET_VARS];       /* <= max_value (-5) */
    int32_t obj_param[NYX_HIP_MAX_TARGET_OBJS];          /* enum nyx_hip_frame_param (0 .. 24) */
    double obj_desired[NYX_HIP_MAX_TARGET_OBJS];
    double obj_tolerance[NYX_HIP_MAX_TARGET_OBJS];       /* finite, >= 0 */
    double obj_mult[NYX_HIP_MAX_TARGET_OBJS];            /* the reference's multiplicative_factor (1) */
    double obj_add[NYX_HIP_MAX_TARGET_OBJS];             /* additive_factor (0) */
    int32_t n_chain;                                     /* the objective target; 0 = the integration centre itself */
    int32_t chain_segment[NYX_HIP_MAX_CHAIN];            /* indices into the context's segments */
    int32_t chain_sign[NYX_HIP_MAX_CHAIN];               /* +1 / -1 */
    int32_t _pad;
    double mu_km3_s2;                                    /* of the objective target; finite, > 0 */
    int64_t correction_epoch_ns, achievement_epoch_ns;
} nyx_hip_target_query_t;

typedef struct nyx_hip_target_result {
    int32_t *status;           /* [n] enum nyx_hip_target_status */
    int32_t *iterations;       /* [n] the iteration at which the run ended */
    double *correction;        /* [n_vars * n]: correction[j * n + i], the run's total */
    double *achieved_errors;   /* [n_objs * n]: achieved_errors[o * n + i], the run's last err */
    nyx_hip_states_t corrected;  /* the state at the correction epoch with the correction applied; epoch and the six Cartesian arrays mandatory, the others written where given */
    nyx_hip_states_t achieved;   /* the nominal's last final state, about the context's centre; likewise */
    int32_t iterations_run;    /* OUT: propagation rounds of the loop = the largest run's iteration + 1 */
    int32_t _pad;
} nyx_hip_target_result_t;

/* Host arrays.  Refused before anything is launched, the outputs untouched, with NYX_HIP_RC_BAD_ARG (and a nyx_hip_last_error text)
 * unless another code is named, in this order: a null context, query or result; n_vars or n_objs outside 1..6; iterations outside
 * 0..1000; a correction frame other than inertial or VNC; per variable: an unknown component, a perturbation that is zero or not
 * finite, max_step < 0 (or NaN), max_value < 0, min_value > max_value, a position variable together with VNC (the reference's
 * FrameError); per objective: an unknown parameter, a tolerance that is not finite or not >= 0; n_chain outside 0..4, a segment
 * index < 0, a sign that is not +1 / -1; mu_km3_s2 not finite and > 0; `in` without its epoch or Cartesian arrays; a NULL output
 * array; in->stm != NULL: NYX_HIP_RC_UNSUPPORTED (that is the hyperdual targeter); then, of the context: a segment index that is not
 * one of its segments, and NYX_HIP_RC_UNSUPPORTED for a context that carries STMs or was built with an integration-frame swap. */
int32_t nyx_hip_target_batch(nyx_hip_ctx *ctx, const nyx_hip_states_t *in, const nyx_hip_target_query_t *q, nyx_hip_target_result_t *res);

/* Device arrays (in's, res's), on `hip_stream` (a hipStream_t; NULL = the default stream), ordered after the context's earlier
 * launches.  NOT asynchronous: the stream is awaited once per iteration (see THE LOOP); the results are complete on return. */
int32_t nyx_hip_target_batch_device(nyx_hip_ctx *ctx, const nyx_hip_states_t *in, const nyx_hip_target_query_t *q, nyx_hip_target_result_t *res,
                                    void *hip_stream);

/* Layout check for mirrors: 0 = sizeof(nyx_hip_target_query_t), 1 = NYX_HIP_TARGET_VERSION, 2 = NYX_HIP_TGT_STATUS_COUNT,
 * 3 = NYX_HIP_MAX_TARGET_VARS, 4 = sizeof(nyx_hip_target_result_t), 5 = NYX_HIP_MAX_TARGET_OBJS; anything else -1. */
int32_t nyx_hip_target_sizeof(int32_t which);

#ifdef __cplusplus
}
#endif
#endif /* NYX_HIP_TARGET_H */
