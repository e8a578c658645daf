// eclipse_dev.h — what the eclipse kernel (eclipse_kernel.hip) evaluates per sample, written so that the SAME TEXT compiles for the
// device and for the host (ECL_FN): tests/cxx/eclipse_host_check.cpp runs the very code of the kernel on the CPU.  A stand-alone
// restatement, on purpose, of two pieces of the propagator's translation units (pk_epoch_data.h: `cheby_eval`, pk_force_models.h:
// `occultation_pct`), which stay untouched - their code objects and budgets do not move with this report:
//   ecl_cheby       SPK type 2 by the Clenshaw recurrence, the rolled form: w0 = cf[j] + (two_t * w1 - w2), r = cf[0] + (t * w0 - w1),
//                   honouring DevSeg.stride (the host may have laid the records out sixteen coefficients wide, zero-padded)
//   ecl_occultation anise's Occultation.percentage as oracle/nyx_oracle.c restates it, with the angles it was formed from
// Compile with -ffp-contract=off: the operations are those of the oracle, one rounding each.
#pragma once
#include <math.h>
#include <stdint.h>

#include "devcfg.h"

#if defined(__HIPCC__)
#define ECL_FN static __host__ __device__ __forceinline__
#else
#define ECL_FN static inline
#endif

// Position of one segment at et_s -> r3; NYX_HIP_OK, or NYX_HIP_ERR_EPHEM_RANGE when et_s lies outside the segment (r3 is then
// the clamped record's value: never used).  `records` is the context's table in its DEVICE layout (DevSeg.offset / .stride).
ECL_FN int ecl_cheby(const DevSeg &sg, const double *records, double et_s, double *r3) {
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
        double w0 = 0.0, w1 = 0.0, w2;
        for (int j = nc - 1; j >= 1; --j) {
            w2 = w1;
            w1 = w0;
            w0 = cf[j] + (two_t * w1 - w2);
        }
        r3[c] = cf[0] + (t * w0 - w1);
    }
    return st;
}

ECL_FN double ecl_norm3(const double *v) { return sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); }

// The apparent radius of a disk of `radius_km` seen from `dist_km`; THE QUIRK: nearer than the radius, the radius itself (km)
ECL_FN double ecl_apparent(double radius_km, double dist_km) { return (radius_km >= dist_km) ? radius_km : asin(radius_km / dist_km); }

ECL_FN double ecl_circ_seg_area(double r, double d) { return r * r * acos(d / r) - d * sqrt(r * r - d * d); }

struct EclDisk {   // one body against the light source, as the percentage formula used it
    double fo_p, d_p, pct;
};

// r_eb = observer w.r.t. the body, r_ls = light source w.r.t. the observer, n_ls = |r_ls|, ls_p = ecl_apparent(R_sun, n_ls)
ECL_FN EclDisk ecl_occultation(double ls_p, double n_ls, double r_front_km, const double *r_eb, const double *r_ls) {
    EclDisk o;
    const double n_eb = ecl_norm3(r_eb);
    const double fo_p = ecl_apparent(r_front_km, n_eb);
    const double dot = r_ls[0] * r_eb[0] + r_ls[1] * r_eb[1] + r_ls[2] * r_eb[2];
    const double d_p = acos(-dot / (n_eb * n_ls));
    double pct;
    if (d_p - ls_p > fo_p) {
        pct = 0.0;    // lit
    } else if (fo_p > d_p + ls_p) {
        pct = 100.0;  // umbra
    } else if (fabs(ls_p - fo_p) < d_p && d_p < ls_p + fo_p) {  // penumbra: the lens of two overlapping disks
        const double d1 = (d_p * d_p - ls_p * ls_p + fo_p * fo_p) / (2.0 * d_p);
        const double d2 = (d_p * d_p + ls_p * ls_p - fo_p * fo_p) / (2.0 * d_p);
        const double shadow = ecl_circ_seg_area(fo_p, d1) + ecl_circ_seg_area(ls_p, d2);
        if (shadow != shadow) {
            pct = 100.0;
        } else {
            const double nominal = 3.14159265358979323846 * (ls_p * ls_p);
            pct = 100.0 * shadow / nominal;
        }
    } else {
        pct = 100.0 * (fo_p * fo_p) / (ls_p * ls_p);  // annular
    }
    o.fo_p = fo_p;
    o.d_p = d_p;
    o.pct = pct;
    return o;
}
