// eclipse_dev.h — what the eclipse kernel (eclipse_kernel.hip) evaluates per sample beside the chains (chain_dev.h), written so that the
// SAME TEXT compiles for the device and for the host (ECL_FN): tests/cxx/eclipse_host_check.cpp runs the very code of the kernel on
// the CPU.  A stand-alone restatement, on purpose, of `occultation_pct` of the propagator's pk_force_models.h, which stays untouched:
//   ecl_occultation anise's Occultation.percentage as oracle/nyx_oracle.c restates it, with the angles it was formed from
// Compile with -ffp-contract=off: the operations are those of the oracle, one rounding each.
#pragma once
#include <math.h>
#include <stdint.h>

#include "chain_dev.h"

#define ECL_FN CHAIN_FN

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
