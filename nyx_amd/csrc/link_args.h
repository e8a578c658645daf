// link_args.h — launch arguments of the link kernels (link_kernel.hip), shared with abi.cpp, and what the host works out once per
// call: which intermediates the requested parameters need, and the DISTINCT ephemeris segments of the chains of the bodies that can
// block the line (host and device; no HIP).  The arguments of ric_args.h (two trajectories) joined to those of eclipse_args.h
// (the chains), whose reduction step this report shares.
#pragma once
#include <stdint.h>

#include "../../include/nyx_hip_link.h"
#include "devcfg.h"
#include "eclipse_args.h"   // EclChain, ECL_MAX_USEG, ecl_reduce_chain

static_assert(NYX_HIP_MAX_LINK_BODIES <= 31, "LnkArgs.body_mask holds one bit per body");

// shared intermediates of one sample: each is computed only when a requested parameter needs it
enum {
    LNK_NEED_RHO = 1,     // rho and |rho|
    LNK_NEED_DV = 2,      // v_rx - v_tx
    LNK_NEED_SIGHT = 4,   // the SIGHT test of EVERY body: Visible, ObstructingBody, Clearance
    LNK_NEED_BODY = 8     // the SIGHT test of the bodies named in param_body (LnkArgs.body_mask)
};

struct LnkArgs {
    nyx_hip_traj_t src;   // the receivers, the runs: device pointers, step-major [k * n + i]
    nyx_hip_traj_t ref;   // the transmitter: step-major [k * n_ref + j], j = 0 (n_ref = 1) or i (n_ref = n)
    int64_t n, n_ref;
    int64_t capacity;     // stored samples per run and parameter
    double *values;       // [n_params][capacity][n]
    int32_t *len;         // [n] samples produced
    int64_t *epoch0;      // [n] epoch of sample 0, or NULL
    nyx_hip_link_query_t q;
    const double *records;            // the context's ephemeris records on the device (DevSeg.offset points into it)
    int32_t n_useg;                   // distinct segments of the chains in use, filled by lnk_reduce_chains
    int32_t seg_index[ECL_MAX_USEG];  // which segment of the context each is (first use first)
    DevSeg seg[ECL_MAX_USEG];         // its row of DevCfg.seg: kernel arguments, scalar loads
    EclChain body[NYX_HIP_MAX_LINK_BODIES];
    int32_t need;                     // LNK_NEED_* of q.param[0 .. n_params), filled by the launcher
    int32_t body_mask;                // bit b: a per-body parameter names bodies[b]
    int64_t sample0;                  // the first sample of this launch of the evaluation kernel, filled by the launcher
};
// the segment rows and the chains travel as kernel arguments (scalar loads, the same for every lane): the kernel-argument limit
static_assert(sizeof(LnkArgs) <= 4096, "LnkArgs must fit the kernel-argument segment");

static constexpr bool lnk_param_per_body(int32_t param) { return param >= NYX_HIP_LNK_BODY_CLEARANCE && param < NYX_HIP_LNK_COUNT; }

// LNK_NEED_* of one parameter; -1 = not a parameter of enum nyx_hip_link_param
static inline int32_t lnk_param_needs(int32_t param) {
    switch (param) {
    case NYX_HIP_LNK_RANGE: case NYX_HIP_LNK_REFERENCE_DOPPLER: case NYX_HIP_LNK_LOS_X: case NYX_HIP_LNK_LOS_Y: case NYX_HIP_LNK_LOS_Z:
        return LNK_NEED_RHO;
    case NYX_HIP_LNK_RANGE_RATE: return LNK_NEED_RHO | LNK_NEED_DV;
    case NYX_HIP_LNK_RELATIVE_SPEED: return LNK_NEED_DV;
    case NYX_HIP_LNK_VISIBLE: case NYX_HIP_LNK_OBSTRUCTING_BODY: case NYX_HIP_LNK_CLEARANCE: return LNK_NEED_SIGHT;
    case NYX_HIP_LNK_BODY_CLEARANCE: case NYX_HIP_LNK_BODY_OBSTRUCTS: return LNK_NEED_BODY;
    default: return -1;
    }
}

// a.need / a.body_mask from a.q (a query check_link_series has accepted)
static inline void lnk_needs(LnkArgs &a) {
    a.need = 0;
    a.body_mask = 0;
    for (int p = 0; p < a.q.n_params; ++p) {
        a.need |= lnk_param_needs(a.q.param[p]);
        if (lnk_param_per_body(a.q.param[p])) a.body_mask |= 1 << a.q.param_body[p];
    }
}

// The chains of a.q.bodies, in order, reduced to their distinct segments (ecl_reduce_chain of eclipse_args.h, body after body): a.n_useg,
// a.seg_index, a.seg (rows of `ctx_seg`, the context's DevCfg.seg), a.body.  a.n_useg == 0 - no body has a chain, the default -
// lets the kernel skip the ephemerides altogether.  Returns false when the chains name more than ECL_MAX_USEG distinct segments,
// which a query check_link_context has accepted cannot.
static inline bool lnk_reduce_chains(LnkArgs &a, const DevSeg *ctx_seg) {
    a.n_useg = 0;
    for (int b = 0; b < a.q.n_bodies; ++b)
        if (!ecl_reduce_chain(a.q.bodies[b], a.body[b], a.n_useg, a.seg_index, a.seg, ctx_seg)) return false;
    return true;
}
