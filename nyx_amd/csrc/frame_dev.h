// frame_dev.h — what the encounter kernel (frame_kernel.hip) evaluates per sample beside the chain (chain_dev.h), written so that the
// SAME TEXT compiles for the device and for the host (FRM_FN): tests/cxx/frame_host_check.cpp runs the very code of the kernel on the
// CPU.  A stand-alone restatement, on purpose, of pieces that stay untouched - their code objects and budgets do not move with this
// report:
//   frm_shared / frm_param   the nineteen parameters of enum nyx_hip_state_param as report_kernel.hip evaluates them (that kernel's
//                  rep_shared / rep_value live in its translation unit; the needs come from report_args.h, which is included)
//   frm_bplane     BdotT / BdotR after cosmic/bplane.rs, as include/nyx_hip_frame.h writes them out
// The formulas are restated on the host by nyx_amd/frames.py, which is what the kernel is tested against.
// Compile with -ffp-contract=off: one rounding per operation.
#pragma once
#include <math.h>
#include <stdint.h>

#include "chain_dev.h"
#include "frame_args.h"

#define FRM_FN CHAIN_FN

constexpr double FRM_DEG = 180.0 / 3.14159265358979323846;  // np.degrees: x * (180 / pi)

// `_wrap360` of params.py (rep_wrap360 of report_kernel.hip)
FRM_FN double frm_wrap360(double a) {
    double m = fmod(a, 360.0);
    if (m != 0.0) {
        if (m < 0.0) m = m + 360.0;
    } else {
        m = 0.0;
    }
    return m < 0.0 ? m + 360.0 : m;
}

struct FrmShared {  // what several parameters of one sample have in common
    double rmag, vmag, h0, h1, h2, hmag, energy, sma, e0, e1, e2, ecc, bt, br;
};

// BdotT / BdotR of a state whose shared intermediates (all six REP_NEED_*) are in `s`; NaN where ecc <= 1 (not a hyperbola)
FRM_FN void frm_bplane(FrmShared &s) {
    const double inv_e = 1.0 / s.ecc;
    const double eh0 = s.e0 / s.ecc, eh1 = s.e1 / s.ecc, eh2 = s.e2 / s.ecc;
    const double hh0 = s.h0 / s.hmag, hh1 = s.h1 / s.hmag, hh2 = s.h2 / s.hmag;
    const double n0 = hh1 * eh2 - hh2 * eh1, n1 = hh2 * eh0 - hh0 * eh2, n2 = hh0 * eh1 - hh1 * eh0;
    const double f = sqrt(1.0 - inv_e * inv_e);
    const double s0 = eh0 / s.ecc + f * n0, s1 = eh1 / s.ecc + f * n1, s2 = eh2 / s.ecc + f * n2;
    const double smag = sqrt((s0 * s0 + s1 * s1) + s2 * s2);
    const double sh0 = s0 / smag, sh1 = s1 / smag, sh2 = s2 / smag;
    const double b = fabs(s.sma) * sqrt(s.ecc * s.ecc - 1.0);
    const double B0 = b * (f * eh0 - inv_e * n0), B1 = b * (f * eh1 - inv_e * n1), B2 = b * (f * eh2 - inv_e * n2);
    // t = s^ x (0, 0, 1) = (s^_1, -s^_0, 0)
    const double t0 = sh1, t1 = -sh0;
    const double tmag = sqrt(t0 * t0 + t1 * t1);
    const double th0 = t0 / tmag, th1 = t1 / tmag, th2 = 0.0 / tmag;
    const double r0 = sh1 * th2 - sh2 * th1, r1 = sh2 * th0 - sh0 * th2, r2 = sh0 * th1 - sh1 * th0;
    const bool hyp = s.ecc > 1.0;
    s.bt = hyp ? (B0 * th0 + B1 * th1) + B2 * th2 : __builtin_nan("");
    s.br = hyp ? (B0 * r0 + B1 * r1) + B2 * r2 : __builtin_nan("");
}

// `need` is the same for every lane (a kernel argument): scalar branches
FRM_FN void frm_shared(int32_t need, double mu, const double y[6], FrmShared &s) {
    if (need & REP_NEED_R) s.rmag = sqrt((y[0] * y[0] + y[1] * y[1]) + y[2] * y[2]);
    if (need & REP_NEED_V) s.vmag = sqrt((y[3] * y[3] + y[4] * y[4]) + y[5] * y[5]);
    if (need & REP_NEED_H) {
        s.h0 = y[1] * y[5] - y[2] * y[4];
        s.h1 = y[2] * y[3] - y[0] * y[5];
        s.h2 = y[0] * y[4] - y[1] * y[3];
        s.hmag = sqrt((s.h0 * s.h0 + s.h1 * s.h1) + s.h2 * s.h2);
    }
    if (need & REP_NEED_ENERGY) s.energy = 0.5 * s.vmag * s.vmag - mu / s.rmag;
    if (need & REP_NEED_SMA) s.sma = -mu / (2.0 * s.energy);
    if (need & REP_NEED_EVEC) {
        const double k = s.vmag * s.vmag - mu / s.rmag;
        const double rv = (y[0] * y[3] + y[1] * y[4]) + y[2] * y[5];
        s.e0 = (k * y[0] - rv * y[3]) / mu;
        s.e1 = (k * y[1] - rv * y[4]) / mu;
        s.e2 = (k * y[2] - rv * y[5]) / mu;
        s.ecc = sqrt((s.e0 * s.e0 + s.e1 * s.e1) + s.e2 * s.e2);
    }
    if (need & FRM_NEED_BPLANE) frm_bplane(s);
}

// `param` is the same for every lane (a kernel argument): the chain below is a scalar branch
FRM_FN double frm_param(int32_t param, double mu, const double y[6], const FrmShared &s) {
    switch (param) {
    case NYX_HIP_SP_X: return y[0];
    case NYX_HIP_SP_Y: return y[1];
    case NYX_HIP_SP_Z: return y[2];
    case NYX_HIP_SP_VX: return y[3];
    case NYX_HIP_SP_VY: return y[4];
    case NYX_HIP_SP_VZ: return y[5];
    case NYX_HIP_SP_RMAG: return s.rmag;
    case NYX_HIP_SP_VMAG: return s.vmag;
    case NYX_HIP_SP_HMAG: return s.hmag;
    case NYX_HIP_SP_ENERGY: return s.energy;
    case NYX_HIP_SP_SEMI_MAJOR_AXIS: return s.sma;
    case NYX_HIP_SP_ECCENTRICITY: return s.ecc;
    case NYX_HIP_SP_APOAPSIS_RADIUS: return s.sma * (1.0 + s.ecc);
    case NYX_HIP_SP_PERIAPSIS_RADIUS: return s.sma * (1.0 - s.ecc);
    case NYX_HIP_SP_PERIOD: return 6.283185307179586 * sqrt(pow(s.sma, 3.0) / mu);
    case NYX_HIP_SP_INCLINATION: {
        const double c = s.h2 / s.hmag;
        return acos(c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c)) * FRM_DEG;  // (a NaN passes the clip, as in np.clip)
    }
    case NYX_HIP_SP_RAAN: return frm_wrap360(atan2(s.h0, -s.h1) * FRM_DEG);  // node n = z x h = (-h1, h0, 0)
    case NYX_HIP_SP_AOP: {
        const double n0 = -s.h1, n1 = s.h0, n2 = 0.0;
        const double cosw = (n0 * s.e0 + n1 * s.e1) + n2 * s.e2;
        const double c0 = n1 * s.e2 - n2 * s.e1, c1 = n2 * s.e0 - n0 * s.e2, c2 = n0 * s.e1 - n1 * s.e0;
        const double sinw = ((c0 * s.h0 + c1 * s.h1) + c2 * s.h2) / s.hmag;
        return frm_wrap360(atan2(sinw, cosw) * FRM_DEG);
    }
    case NYX_HIP_SP_TRUE_ANOMALY: {
        const double cost = (s.e0 * y[0] + s.e1 * y[1]) + s.e2 * y[2];
        const double c0 = s.e1 * y[2] - s.e2 * y[1], c1 = s.e2 * y[0] - s.e0 * y[2], c2 = s.e0 * y[1] - s.e1 * y[0];
        const double sint = ((c0 * s.h0 + c1 * s.h1) + c2 * s.h2) / s.hmag;
        return frm_wrap360(atan2(sint, cost) * FRM_DEG);
    }
    case NYX_HIP_FRM_C3: return s.vmag * s.vmag - 2.0 * mu / s.rmag;
    case NYX_HIP_FRM_B_DOT_T: return s.bt;
    case NYX_HIP_FRM_B_DOT_R: return s.br;
    case NYX_HIP_FRM_B_ANGLE: {
        const double a = atan2(s.br, s.bt) * FRM_DEG;
        return a == -180.0 ? 180.0 : a;   // (-180, 180]
    }
    case NYX_HIP_FRM_B_MAGNITUDE: return sqrt(s.bt * s.bt + s.br * s.br);
    case NYX_HIP_FRM_V_INFINITY: return s.ecc > 1.0 ? sqrt(s.vmag * s.vmag - 2.0 * mu / s.rmag) : __builtin_nan("");
    default: return __builtin_nan("");
    }
}

// One parameter of one state about a centre of `mu`: the per-sample definition (frames.frame_value on a translated state)
FRM_FN double frm_value(int32_t param, const double *rv6, double mu) {
    const int32_t need = frm_param_needs(param);
    if (need < 0) return __builtin_nan("");
    FrmShared s;
    frm_shared(need, mu, rv6, s);
    return frm_param(param, mu, rv6, s);
}
