// chain_args.h - the ephemeris chain on the host (host and device text; no HIP, no process state).  A chain is up to
// NYX_HIP_MAX_CHAIN pairs (segment of the context, sign +1 / -1) whose signed sum of SPK type 2 segments, in chain order and from
// zero, is a body's state about the integration centre; the empty chain is the centre itself.  The eclipse, encounter, link, Lambert
// and targeter queries all carry one or more (n_chain / chain_segment[] / chain_sign[]); this is what they share:
//   ChainView, chain_view      the three members of any of the public layouts
//   check_chain                what is refused of a chain from the query alone
//   check_chain_context        what a chain asks OF the context (DevCfg.n_seg), checked once the query itself is sound
//   frame_swap_refusal         the one refusal that is not a bad argument: a context built with an integration-frame swap
//   ReducedChain, reduce_chain a chain over the DISTINCT segments of a call: the series kernels evaluate each once per sample
//   ResolvedChain, resolve_chain   a chain with its segment rows, link by link: the kernels that evaluate a chain at few epochs
// The device side is chain_dev.h.
#pragma once
#include <stdint.h>

#include "devcfg.h"
#include "refusal.h"

struct ChainView {
    int32_t n;
    const int32_t *segment, *sign;
};
template <typename T>
inline ChainView chain_view(const T &c) { return {c.n_chain, c.chain_segment, c.chain_sign}; }

// `who` names the chain inside the query (`light`, `bodies[2]`, `dep`); "" for a query with one chain of its own
inline Refusal check_chain(const char *name, const char *who, ChainView c, int min_chain) {
    const char *dot = *who ? "." : "";
    if (c.n < min_chain || c.n > NYX_HIP_MAX_CHAIN)
        return bad_arg("%s: %s%sn_chain = %d, %d .. %d segments", name, who, dot, c.n, min_chain, NYX_HIP_MAX_CHAIN);
    for (int k = 0; k < c.n; ++k) {
        if (c.segment[k] < 0) return bad_arg("%s: %s%schain_segment[%d] = %d is not a segment of the context", name, who, dot, k, c.segment[k]);
        if (c.sign[k] != 1 && c.sign[k] != -1) return bad_arg("%s: %s%schain_sign[%d] = %d, +1 or -1", name, who, dot, k, c.sign[k]);
    }
    return {};
}
// (of a chain check_chain has accepted)
inline Refusal check_chain_context(const char *name, const char *who, ChainView c, int n_seg) {
    const char *dot = *who ? "." : "";
    for (int k = 0; k < c.n; ++k)
        if (c.segment[k] >= n_seg)
            return bad_arg("%s: %s%schain_segment[%d] = %d is not a segment of the context (0 .. %d)", name, who, dot, k, c.segment[k], n_seg - 1);
    return {};
}
// The chains of such a context (state_frame_body != 0) are not those of the states it stores; `closing` says what that means for the entry
inline Refusal frame_swap_refusal(const char *name, const char *closing) {
    Refusal r = bad_arg("%s: the context was built with an integration-frame swap (state_frame_body != 0): %s", name, closing);
    r.rc = NYX_HIP_RC_UNSUPPORTED;
    return r;
}

// A chain as a series kernel walks it: state = sum_k sign[k] * (vector of distinct segment useg[k]), in chain order
struct ReducedChain {
    int32_t n_chain;
    int32_t useg[NYX_HIP_MAX_CHAIN];  // indices into the call's distinct segments (seg_index / seg of its *Args)
    double sign[NYX_HIP_MAX_CHAIN];
};
// One chain over the distinct segments found so far: n_useg of them, seg_index[u] the segment of the context, seg[u] its row of
// `ctx_seg` (the context's DevCfg.seg), first use first.  The chain order is kept, so the sums are those of the oracle.  Returns
// false when the chain would name more than `max_useg` distinct segments.
static inline bool reduce_chain(ChainView src, ReducedChain &dst, int32_t &n_useg, int32_t *seg_index, DevSeg *seg, int max_useg,
                                const DevSeg *ctx_seg) {
    dst.n_chain = src.n;
    for (int k = 0; k < NYX_HIP_MAX_CHAIN; ++k) { dst.useg[k] = 0; dst.sign[k] = 0.0; }
    for (int k = 0; k < src.n; ++k) {
        int u = 0;
        while (u < n_useg && seg_index[u] != src.segment[k]) ++u;
        if (u == n_useg) {
            if (n_useg == max_useg) return false;
            seg_index[u] = src.segment[k];
            seg[u] = ctx_seg[src.segment[k]];
            ++n_useg;
        }
        dst.useg[k] = u;
        dst.sign[k] = (double)src.sign[k];
    }
    return true;
}

// A chain with its segment rows: state = sum_k sign[k] * (state of seg[k]), in chain order, from zero.  The rows travel as kernel
// arguments (scalar loads, the same for every lane).
struct ResolvedChain {
    int32_t n_chain, _pad;
    double sign[NYX_HIP_MAX_CHAIN];
    DevSeg seg[NYX_HIP_MAX_CHAIN];
};
static inline ResolvedChain resolve_chain(ChainView c, const DevSeg *ctx_seg) {
    ResolvedChain out = {};
    out.n_chain = c.n;
    for (int k = 0; k < c.n; ++k) {
        out.sign[k] = (double)c.sign[k];
        out.seg[k] = ctx_seg[c.segment[k]];
    }
    return out;
}
