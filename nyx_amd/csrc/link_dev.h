// link_dev.h — what the link kernel (link_kernel.hip) evaluates per sample, written so that the SAME TEXT compiles for the device and
// for the host (LNK_FN): tests/cxx/link_host_check.cpp runs the very code of the kernel's second pass on the CPU.  No HIP includes,
// nothing read from the process.
//   lnk_segments   every DISTINCT segment of the chains in use once, at one epoch (frm_cheby_pv of chain_dev.h, position only), parked
//                  where the caller says: base[u * su + c * sc] is component c of distinct segment u (the kernel: a column of LDS per
//                  lane, written and read by that lane alone; the host check: a plain array)
//   lnk_sight      Vallado's SIGHT test of one body, as include/nyx_hip_link.h states it
//   lnk_sample     the second pass of one sample: the shared intermediates `need` names, the chains summed in chain order (chain_sum), the SIGHT
//                  test per body, every requested parameter handed to `put(p, value)`
// nyx_amd/links.py restates this operation for operation (sums of three as ((a0 + a1) + a2)); only + - x /, sqrt and comparisons:
// compile with -ffp-contract=off and the two agree to the last bit.
#pragma once
#include <math.h>
#include <stdint.h>

#include "chain_dev.h"
#include "link_args.h"

#define LNK_FN CHAIN_FN
#define LNK_ROLLED CHAIN_ROLLED

// NYX_HIP_OK, or NYX_HIP_ERR_EPHEM_RANGE when et_s lies outside one of the segments (what was parked is then never used).  Nothing is
// evaluated when no body has a chain (n_useg == 0).
LNK_FN int lnk_segments(const LnkArgs &a, double et_s, double *base, int su, int sc) {
    int st = NYX_HIP_OK;
    LNK_ROLLED
    for (int u = 0; u < a.n_useg; ++u) {
        double p[3];
        const int s1 = frm_cheby_pv(a.seg[u], a.records, et_s, false, p, nullptr);
        if (s1) st = s1;
        base[u * su] = p[0];
        base[u * su + sc] = p[1];
        base[u * su + 2 * sc] = p[2];
    }
    return st;
}

struct LnkSight {
    double clearance;   // sqrt(d2) - R
    bool obstructs;
};

LNK_FN double lnk_dot3(const double *a, const double *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// rx / tx: receiver and transmitter, b: the body, all w.r.t. the context's centre.  Coincident spacecraft: tau = 0 / 0 is NaN, every
// comparison with it false - not obstructed, the clearance NaN.  Not guarded.
LNK_FN LnkSight lnk_sight(const double *rx, const double *tx, const double *b, double radius_km) {
    const double r1[3] = {rx[0] - b[0], rx[1] - b[1], rx[2] - b[2]};
    const double r2[3] = {tx[0] - b[0], tx[1] - b[1], tx[2] - b[2]};
    const double r1sq = lnk_dot3(r1, r1), r2sq = lnk_dot3(r2, r2), d = lnk_dot3(r1, r2);
    const double tau = (r1sq - d) / ((r1sq + r2sq) - 2.0 * d);
    const double d2 = tau < 0.0 ? r1sq : (tau > 1.0 ? r2sq : (1.0 - tau) * r1sq + d * tau);
    LnkSight s;
    s.obstructs = tau >= 0.0 && tau <= 1.0 && d2 <= radius_km * radius_km;
    s.clearance = sqrt(d2) - radius_km;
    return s;
}

// rx6 / tx6: the two interpolated states; base / su / sc: where lnk_segments parked the segments of THIS sample.  `put(p, value)` is
// called once for every p < n_params.  `need`, `body_mask`, `param[p]`, `param_body[p]` and the chains are the same for every lane.
template <typename Put>
LNK_FN void lnk_sample(const LnkArgs &a, const double *rx6, const double *tx6, const double *base, int su, int sc, Put put) {
    const double qnan = __builtin_nan("");
    double rho[3] = {qnan, qnan, qnan}, dv[3] = {qnan, qnan, qnan}, range = qnan;
    if (a.need & LNK_NEED_RHO) {
        for (int c = 0; c < 3; ++c) rho[c] = rx6[c] - tx6[c];
        range = sqrt(lnk_dot3(rho, rho));
    }
    if (a.need & LNK_NEED_DV)
        for (int c = 0; c < 3; ++c) dv[c] = rx6[3 + c] - tx6[3 + c];
    double first = -1.0, clearance = __builtin_inf();   // the first body that obstructs; the smallest clearance (strict <: a NaN never wins)
    if (a.need & (LNK_NEED_SIGHT | LNK_NEED_BODY)) {
        LNK_ROLLED
        for (int b = 0; b < a.q.n_bodies; ++b) {
            if (!(a.need & LNK_NEED_SIGHT) && !((a.body_mask >> b) & 1)) continue;
            const EclChain &ch = a.body[b];
            double pos[3];   // (an empty chain: the centre itself)
            chain_sum<3>(ch, base, su, sc, pos);
            const LnkSight s = lnk_sight(rx6, tx6, pos, ch.radius_km);
            if (s.obstructs && first < 0.0) first = (double)b;
            if (s.clearance < clearance) clearance = s.clearance;
            if ((a.body_mask >> b) & 1) {
                LNK_ROLLED
                for (int p = 0; p < a.q.n_params; ++p) {
                    if (!lnk_param_per_body(a.q.param[p]) || a.q.param_body[p] != b) continue;
                    put(p, a.q.param[p] == NYX_HIP_LNK_BODY_CLEARANCE ? s.clearance : (s.obstructs ? 1.0 : 0.0));
                }
            }
        }
    }
    LNK_ROLLED
    for (int p = 0; p < a.q.n_params; ++p) {
        double val = qnan;
        switch (a.q.param[p]) {   // (a scalar branch)
        case NYX_HIP_LNK_RANGE: val = range; break;
        case NYX_HIP_LNK_RANGE_RATE: val = lnk_dot3(rho, dv) / range; break;
        case NYX_HIP_LNK_REFERENCE_DOPPLER: val = lnk_dot3(rho, rx6 + 3) / range; break;
        case NYX_HIP_LNK_VISIBLE: val = first < 0.0 ? 1.0 : 0.0; break;
        case NYX_HIP_LNK_OBSTRUCTING_BODY: val = first; break;
        case NYX_HIP_LNK_CLEARANCE: val = clearance; break;
        case NYX_HIP_LNK_RELATIVE_SPEED: val = sqrt(lnk_dot3(dv, dv)); break;
        case NYX_HIP_LNK_LOS_X: val = rho[0] / range; break;
        case NYX_HIP_LNK_LOS_Y: val = rho[1] / range; break;
        case NYX_HIP_LNK_LOS_Z: val = rho[2] / range; break;
        default: continue;       // a per-body parameter: written above
        }
        put(p, val);
    }
}
