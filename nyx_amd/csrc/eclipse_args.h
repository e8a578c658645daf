// eclipse_args.h — launch arguments of the eclipse kernels (eclipse_kernel.hip), shared with abi.cpp, and what the host works out
// once per call: which intermediates the requested parameters need, and the chains of the light source and the shadow bodies reduced
// to their distinct segments (chain_args.h) (host and device; no HIP).
#pragma once
#include <stdint.h>

#include "../../include/nyx_hip_eclipse.h"
#include "chain_args.h"
#include "devcfg.h"

// shared intermediates of one sample: each is computed only when a requested parameter needs it
enum {
    ECL_NEED_SUN_RADIUS = 1,  // ls_p (one asin)
    ECL_NEED_MODEL = 2,       // the percentage of EVERY body: the shadow model's maximum
    ECL_NEED_BODY = 4         // the disk of the bodies named in param_body (EclArgs.body_mask)
};

// A context holds at most DEV_MAX_SEG segments (ctx_build.h refuses more), so a query has no more distinct ones
#define ECL_MAX_USEG DEV_MAX_SEG
static_assert(ECL_MAX_USEG <= NYX_HIP_MAX_SEGMENTS, "the distinct segments of a query are segments of the configuration");

// The chain of a body with a disk (useg: indices into EclArgs.seg / LnkArgs.seg)
struct EclChain : ReducedChain {
    double radius_km;
};
static_assert(sizeof(EclChain) == sizeof(ReducedChain) + sizeof(double), "the radius follows the signs without padding");

struct EclArgs {
    nyx_hip_traj_t src;   // device pointers, step-major [k * n + i]
    int64_t n;            // trajectories
    int64_t capacity;     // stored samples per trajectory and parameter
    double *values;       // [n_params][capacity][n]
    int32_t *len;         // [n] samples produced
    nyx_hip_ecl_query_t q;
    const double *records;            // the context's ephemeris records on the device (DevSeg.offset points into it)
    int32_t n_useg;                   // distinct segments of the chains in use, filled by ecl_reduce_chains
    int32_t seg_index[ECL_MAX_USEG];  // which segment of the context each is (first use first)
    DevSeg seg[ECL_MAX_USEG];         // its row of DevCfg.seg: kernel arguments, scalar loads
    EclChain light, body[NYX_HIP_MAX_ECL_BODIES];
    int32_t need;                     // ECL_NEED_* of q.param[0 .. n_params), filled by the launcher
    int32_t body_mask;                // bit b: a per-body parameter names bodies[b]
    int64_t sample0;                  // the first sample of this launch of the evaluation kernel, filled by the launcher
};
// the segment rows and the chains travel as kernel arguments (scalar loads, the same for every lane): the kernel-argument limit
static_assert(sizeof(EclArgs) <= 4096, "EclArgs must fit the kernel-argument segment");

static constexpr bool ecl_param_per_body(int32_t param) { return param >= NYX_HIP_ECL_BODY_OCCULTATION && param < NYX_HIP_ECL_COUNT; }

// ECL_NEED_* of one parameter; -1 = not a parameter of enum nyx_hip_ecl_param
static inline int32_t ecl_param_needs(int32_t param) {
    switch (param) {
    case NYX_HIP_ECL_OCCULTATION: case NYX_HIP_ECL_ILLUMINATION: case NYX_HIP_ECL_STATE: case NYX_HIP_ECL_ECLIPSING_BODY:
        return ECL_NEED_SUN_RADIUS | ECL_NEED_MODEL;
    case NYX_HIP_ECL_SUN_RANGE: return 0;
    case NYX_HIP_ECL_SUN_APPARENT_RADIUS: return ECL_NEED_SUN_RADIUS;
    case NYX_HIP_ECL_BODY_OCCULTATION: case NYX_HIP_ECL_BODY_APPARENT_RADIUS: case NYX_HIP_ECL_BODY_SEPARATION:
    case NYX_HIP_ECL_BODY_PENUMBRA_MARGIN: case NYX_HIP_ECL_BODY_UMBRA_MARGIN:
        return ECL_NEED_SUN_RADIUS | ECL_NEED_BODY;
    default: return -1;
    }
}

// a.need / a.body_mask from a.q (a query check_ecl_series has accepted)
static inline void ecl_needs(EclArgs &a) {
    a.need = 0;
    a.body_mask = 0;
    for (int p = 0; p < a.q.n_params; ++p) {
        a.need |= ecl_param_needs(a.q.param[p]);
        if (ecl_param_per_body(a.q.param[p])) a.body_mask |= 1 << a.q.param_body[p];
    }
}

// The chains of a.q (the light source first, then the bodies in order) reduced to their distinct segments (reduce_chain of
// chain_args.h, body after body): a.n_useg, a.seg_index, a.seg, a.light, a.body.  Earth -> EMB is on the chain of the Sun AND of the
// Moon of an Earth-centred context: it is evaluated once per sample.  Returns false (nothing usable in `a`) when the chains name more
// than ECL_MAX_USEG distinct segments, which a query check_ecl_series has accepted cannot.
// (ecl_reduce_chain is the step of ONE body: the link report, link_args.h, shares it)
static inline bool ecl_reduce_chain(const nyx_hip_ecl_body_t &src, EclChain &dst, int32_t &n_useg, int32_t *seg_index, DevSeg *seg,
                                    const DevSeg *ctx_seg) {
    dst.radius_km = src.mean_radius_km;
    return reduce_chain(chain_view(src), dst, n_useg, seg_index, seg, ECL_MAX_USEG, ctx_seg);
}
static inline bool ecl_reduce_chains(EclArgs &a, const DevSeg *ctx_seg) {
    a.n_useg = 0;
    for (int b = -1; b < a.q.n_bodies; ++b)
        if (!ecl_reduce_chain(b < 0 ? a.q.light : a.q.bodies[b], b < 0 ? a.light : a.body[b], a.n_useg, a.seg_index, a.seg, ctx_seg)) return false;
    return true;
}
