// frame_args.h — launch arguments of the encounter kernels (frame_kernel.hip), shared with abi.cpp, and what the host works out once
// per call: which intermediates the requested parameters need, and the DISTINCT ephemeris segments of the target's chain (host and
// device; no HIP).  The reduction is reduce_chain of chain_args.h, for the ONE chain of this report.
#pragma once
#include <stdint.h>

#include "../../include/nyx_hip_frame.h"
#include "chain_args.h"
#include "devcfg.h"
#include "report_args.h"   // REP_NEED_*, report_param_needs: codes 0 .. 18 are enum nyx_hip_state_param

// what one sample evaluates, each only when a requested parameter needs it: the REP_NEED_* intermediates of report_args.h (the low
// bits, as report_param_needs names them) and, above them,
enum {
    FRM_NEED_VELOCITY = 64,   // anything but X / Y / Z / Rmag: the companion recurrence of the body's velocity
    FRM_NEED_ELEMENTS = 128,  // an intermediate of the translated state (one of the REP_NEED_* bits is set)
    FRM_NEED_BPLANE = 256     // BdotT / BdotR
};
static_assert((REP_NEED_R | REP_NEED_V | REP_NEED_H | REP_NEED_ENERGY | REP_NEED_SMA | REP_NEED_EVEC) < FRM_NEED_VELOCITY, "the two bit sets are disjoint");

// There is one chain here: its distinct segments are no more than its links
#define FRM_MAX_USEG NYX_HIP_MAX_CHAIN

struct FrmArgs {
    nyx_hip_traj_t src;   // device pointers, step-major [k * n + i]
    int64_t n;            // trajectories
    int64_t capacity;     // stored samples per trajectory and parameter
    double *values;       // [n_params][capacity][n]
    int32_t *len;         // [n] samples produced
    nyx_hip_frame_query_t q;
    const double *records;            // the context's ephemeris records on the device (DevSeg.offset points into it)
    int32_t n_useg;                   // distinct segments of the chain, filled by frm_reduce_chain
    int32_t seg_index[FRM_MAX_USEG];  // which segment of the context each is (first use first)
    DevSeg seg[FRM_MAX_USEG];         // its row of DevCfg.seg: kernel arguments, scalar loads
    ReducedChain chain;               // (useg: indices into seg)
    int32_t need;                     // FRM_NEED_* | REP_NEED_* of q.param[0 .. n_params), filled by the launcher
    int64_t sample0;                  // the first sample of this launch of the evaluation kernel, filled by the launcher
};
// the segment rows and the chain travel as kernel arguments (scalar loads, the same for every lane): the kernel-argument limit
static_assert(sizeof(FrmArgs) <= 4096, "FrmArgs must fit the kernel-argument segment");

// FRM_NEED_* | REP_NEED_* of one parameter; -1 = not a parameter of enum nyx_hip_frame_param
static inline int32_t frm_param_needs(int32_t param) {
    const int32_t hyperbola = REP_NEED_R | REP_NEED_V | REP_NEED_EVEC;   // (ecc decides whether the value exists)
    int32_t k;
    switch (param) {
    case NYX_HIP_FRM_C3: k = REP_NEED_R | REP_NEED_V; break;
    case NYX_HIP_FRM_V_INFINITY: k = hyperbola; break;
    case NYX_HIP_FRM_B_DOT_T: case NYX_HIP_FRM_B_DOT_R: case NYX_HIP_FRM_B_ANGLE: case NYX_HIP_FRM_B_MAGNITUDE:
        k = hyperbola | REP_NEED_H | REP_NEED_ENERGY | REP_NEED_SMA | FRM_NEED_BPLANE;
        break;
    default:
        k = report_param_needs(param);
        if (k < 0) return -1;
    }
    if (k) k |= FRM_NEED_ELEMENTS;
    if (k & ~(REP_NEED_R | FRM_NEED_ELEMENTS)) k |= FRM_NEED_VELOCITY;
    if (param == NYX_HIP_SP_VX || param == NYX_HIP_SP_VY || param == NYX_HIP_SP_VZ) k |= FRM_NEED_VELOCITY;
    return k;
}

// a.need from a.q (a query check_frame_series has accepted)
static inline void frm_needs(FrmArgs &a) {
    a.need = 0;
    for (int p = 0; p < a.q.n_params; ++p) a.need |= frm_param_needs(a.q.param[p]);
}

// The chain of a.q reduced to its distinct segments: a.n_useg, a.seg_index, a.seg, a.chain (n_chain <= FRM_MAX_USEG: always room)
static inline void frm_reduce_chain(FrmArgs &a, const DevSeg *ctx_seg) {
    a.n_useg = 0;
    reduce_chain(chain_view(a.q), a.chain, a.n_useg, a.seg_index, a.seg, FRM_MAX_USEG, ctx_seg);
}
