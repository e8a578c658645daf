// chain_dev.h - the ephemeris chain on the device, written so that the SAME TEXT compiles for the device and for the host
// (CHAIN_FN): the tests/cxx/*_host_check.cpp programs run the very code of the kernels on the CPU.  A stand-alone restatement, on
// purpose, of the propagator's `cheby_eval` / `cheby_eval_pv` (pk_epoch_data.h), which stay untouched - the propagator's code objects
// and budgets do not move with the reports:
//   frm_cheby_pv     SPK type 2 with the derivative, as oracle/nyx_oracle.c restates CHBINT (`cheby_eval_pv`): the rolled Clenshaw
//                    recurrence w0 = cf[j] + (two_t * w1 - w2) with its companion d0 = (2 * w1 + two_t * d1) - d2,
//                    r = cf[0] + (t * w0 - w1), v = ((w0 + t * d0) - d1) / radius; honours DevSeg.stride (the host may have laid the
//                    records out sixteen coefficients wide, zero-padded)
//   chain_sum        the signed sum of PARKED distinct segments along a ReducedChain, in chain order, from +0
//   chain_pv         a ResolvedChain evaluated and summed at one epoch
// nyx_amd/chains.py restates these operation for operation.  Compile with -ffp-contract=off: one rounding per operation.
#pragma once
#include <math.h>
#include <stdint.h>

#include "chain_args.h"

#if defined(__HIPCC__)
#define CHAIN_FN static __host__ __device__ __forceinline__
#define CHAIN_ROLLED _Pragma("unroll 1")   // one copy of the body: the trip count and what the body branches on are scalars
#define CHAIN_UNROLL _Pragma("unroll")
#else
#define CHAIN_FN static inline
#define CHAIN_ROLLED
#define CHAIN_UNROLL
#endif

// (the name is the encounter report's, where the evaluator with the `with_v` switch came from)
// Position and (with_v) velocity of one segment at et_s -> r3, v3; NYX_HIP_OK, or NYX_HIP_ERR_EPHEM_RANGE when et_s lies outside
// the segment (r3 / v3 are then the clamped record's: never used).  `records` is the context's table in its DEVICE layout
// (DevSeg.offset / .stride).  `with_v` is the same for every lane; without it v3 is left alone (it may be null) and the companion
// recurrence is not run.
CHAIN_FN int frm_cheby_pv(const DevSeg &sg, const double *records, double et_s, bool with_v, double *r3, double *v3) {
    const double rel = (et_s - sg.init_et) / sg.interval;
    const double fl = floor(rel);
    int st = NYX_HIP_OK;
    // (compared as doubles: an epoch far outside the segment must not overflow the conversion)
    if (!(fl >= 0.0) || fl > (double)sg.n_rec || (fl == (double)sg.n_rec && et_s > sg.end_et)) st = NYX_HIP_ERR_EPHEM_RANGE;
    int idx = !(fl >= 0.0) ? 0 : (fl >= (double)sg.n_rec ? sg.n_rec - 1 : (int)fl);
    const int nc = sg.n_coef;
    const int cs = (sg.stride - 2) / 3;  // doubles per component: n_coef, or sixteen when the host padded the record with zeros
    const double *rec = records + sg.offset + (int64_t)idx * sg.stride;
    const double t = (et_s - rec[0]) / rec[1];
    const double two_t = 2.0 * t;
    for (int c = 0; c < 3; ++c) {
        const double *cf = rec + 2 + c * cs;
        double w0 = 0.0, w1 = 0.0, w2, d0 = 0.0, d1 = 0.0, d2;
        if (with_v) {
            for (int j = nc - 1; j >= 1; --j) {
                w2 = w1;
                w1 = w0;
                w0 = cf[j] + (two_t * w1 - w2);
                d2 = d1;
                d1 = d0;
                d0 = (2.0 * w1 + two_t * d1) - d2;
            }
            v3[c] = ((w0 + t * d0) - d1) / rec[1];
        } else {
            for (int j = nc - 1; j >= 1; --j) {
                w2 = w1;
                w1 = w0;
                w0 = cf[j] + (two_t * w1 - w2);
            }
        }
        r3[c] = cf[0] + (t * w0 - w1);
    }
    return st;
}

// out[c] = sum_k sign[k] * base[useg[k] * su + c * sc], c < NC, in chain order, from +0 (an empty chain: the centre itself).
// base[u * su + c * sc] is component c of distinct segment u where the caller parked it (a kernel: its lane's column of LDS,
// su = NC * LANES, sc = LANES; a host check: a plain array).  The chain is the same for every lane.
template <int NC>
CHAIN_FN void chain_sum(const ReducedChain &ch, const double *base, int su, int sc, double *out) {
    CHAIN_UNROLL
    for (int c = 0; c < NC; ++c) out[c] = 0.0;
    CHAIN_ROLLED
    for (int k = 0; k < ch.n_chain; ++k) {
        const double sg = ch.sign[k];
        const int u = ch.useg[k];
        CHAIN_UNROLL
        for (int c = 0; c < NC; ++c) out[c] = out[c] + sg * base[u * su + c * sc];
    }
}

// The signed sum of a chain at et_s, in chain order, from zero -> rv6; NYX_HIP_OK, or NYX_HIP_ERR_EPHEM_RANGE of one of its segments
CHAIN_FN int chain_pv(const ResolvedChain &ch, const double *records, double et_s, double rv6[6]) {
    int st = NYX_HIP_OK;
    for (int c = 0; c < 6; ++c) rv6[c] = 0.0;
    CHAIN_ROLLED   // (n_chain is a scalar: one copy of the recurrence)
    for (int k = 0; k < ch.n_chain; ++k) {
        double p[3], pv[3];
        if (const int s1 = frm_cheby_pv(ch.seg[k], records, et_s, true, p, pv)) st = s1;
        for (int c = 0; c < 3; ++c) {
            rv6[c] = rv6[c] + ch.sign[k] * p[c];
            rv6[3 + c] = rv6[3 + c] + ch.sign[k] * pv[c];
        }
    }
    return st;
}
