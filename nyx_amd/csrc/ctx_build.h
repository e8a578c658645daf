// ctx_build.h - what nyx_hip_ctx_create (abi.cpp) builds from a nyx_hip_config_t before it touches a device (host only; abi.cpp,
// tests/cxx/ctx_build_check.cpp): the plain-data validation, the DevCfg's force-model part, the ephemeris record image, the harmonics
// tables of both fields and the role duties the planner (launch_plan.h) charges.
//
// Pure functions of their arguments.  The LDS carve of the kernels (nyx_kernel_lds_bytes, pk_state_lds.h) arrives as a function
// pointer.  No device, no HIP; the tuning arrives resolved (resolve_tuning, abi.cpp).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/nyx_hip.h"
#include "butcher.h"
#include "devcfg.h"
#include "launch_plan.h"

// nyx_kernel_lds_bytes(n_waves, rec_doubles, stm, reuse_fields): LDS bytes of a workgroup (stm: 0 = plain, 1 = D3, 2 = quad layout)
typedef size_t (*LdsBytesFn)(int n_waves, int rec_doubles, int stm, int reuse_fields);

constexpr size_t kRecordsLdsMax = 24 * 1024;  // ephemeris records staged in LDS at most (bytes)
constexpr size_t kKernelLdsMax = 160 * 1024;  // LDS of a whole workgroup layout at most (bytes)

// Whether `rec_doubles` of ephemeris records go into LDS beside the buffers of the given layout.
inline bool records_fit_lds(LdsBytesFn lds_bytes, int rec_doubles, int n_waves, int stm, int reuse_fields) {
    return (size_t)rec_doubles * sizeof(double) <= kRecordsLdsMax && lds_bytes(n_waves, rec_doubles, stm, reuse_fields) <= kKernelLdsMax;
}

// tuning.debug_flags that still select something (nyx_hip.h); the builder refuses every other bit
constexpr uint32_t kLiveDebugFlags = 0x100 | 0x200 | 0x400 | 0x800 | 0x4000 | 0x8000 | 0x10000 | 0x80000 | 0x100000 | 0x2000000 |
                                     0x4000000 | 0x8000000 | 0x20000000;

// nyx_hip_rotation_t -> DevRot (validated by check_rotation() first)
inline void copy_rotation(DevRot &d, const nyx_hip_rotation_t &r) {
    std::memset(&d, 0, sizeof d);
    for (int k = 0; k < 3; ++k) { d.ra[k] = r.ra_deg[k]; d.dec[k] = r.dec_deg[k]; d.w[k] = r.w_deg[k]; }
    d.kind = r.kind; d.n_np = r.n_nut_prec;
    for (int k = 0; k < r.n_nut_prec; ++k) {
        d.np_ang[k][0] = r.nut_prec_angle_deg[k][0]; d.np_ang[k][1] = r.nut_prec_angle_deg[k][1];
        d.np_ra[k] = r.nut_prec_ra[k]; d.np_dec[k] = r.nut_prec_dec[k]; d.np_w[k] = r.nut_prec_w[k];
    }
    d.euler_seg = r.euler_segment;
    for (int k = 0; k < 9; ++k) d.base[k] = r.base_dcm[k];
}
inline const char *check_rotation(const nyx_hip_rotation_t &r, int n_segments) {
    if (r.kind != NYX_HIP_ROT_IAU && r.kind != NYX_HIP_ROT_EULER_CHEBY) return "unknown orientation kind";
    if (r.n_nut_prec < 0 || r.n_nut_prec > NYX_HIP_MAX_NUT_PREC) return "n_nut_prec outside 0..NYX_HIP_MAX_NUT_PREC";
    if (r.kind == NYX_HIP_ROT_EULER_CHEBY && (r.euler_segment < 0 || r.euler_segment >= n_segments)) return "euler_segment is not one of config.segments";
    return nullptr;
}

inline double ns_to_seconds_host(int64_t ns) { return (double)(ns / 1000000000LL) + (double)(ns % 1000000000LL) * 1e-9; }  // Duration::to_seconds, 0 <= ns < 1 century

// GravityField::new (reference dynamics/gravity_field.rs:52-132) re-expressed as the per-column
// entry table the kernel streams (see HarmEntry in devcfg.h).
inline void build_harmonics(const nyx_hip_gravity_field_t *g, std::vector<HarmEntry> &tab, std::vector<ColHdr> &cols,
                            std::vector<int32_t> &col_len, int &n_cols) {
    const int N = g->degree, M = std::min(g->order, g->degree);
    auto C = [&](int n, int m) -> double { return (n < 0 || m < 0 || n > N || m > n || m > M) ? 0.0 : g->c_nm[(size_t)n * (n + 1) / 2 + m]; };
    auto S = [&](int n, int m) -> double { return (n < 0 || m < 0 || n > N || m > n || m > M) ? 0.0 : g->s_nm[(size_t)n * (n + 1) / 2 + m]; };
    auto vr01 = [&](int n, int m) -> double {
        double nf = n, mf = m;
        double v = std::sqrt((nf - mf) * (nf + mf + 1.0));
        return m == 0 ? v / std::sqrt(2.0) : v;
    };
    auto vr11 = [&](int n, int m) -> double {
        double nf = n, mf = m;
        double v = std::sqrt(((2.0 * nf + 1.0) * (nf + mf + 2.0) * (nf + mf + 1.0)) / (2.0 * nf + 3.0));
        return m == 0 ? v / std::sqrt(2.0) : v;
    };
    auto bnm = [&](int n, int m) -> double {
        double nf = n, mf = m;
        return std::sqrt(((2.0 * nf + 1.0) * (2.0 * nf - 1.0)) / ((nf + mf) * (nf - mf)));
    };
    auto cnm = [&](int n, int m) -> double {
        double nf = n, mf = m;
        return std::sqrt(((2.0 * nf + 1.0) * (nf + mf - 1.0) * (nf - mf - 1.0)) / ((nf - mf) * (nf + mf) * (2.0 * nf - 3.0)));
    };
    // diagonal A[n][n]
    std::vector<double> diag(N + 3);
    diag[0] = 1.0;
    for (int n = 1; n <= N + 2; ++n) diag[n] = std::sqrt(1.0 + 1.0 / (2.0 * (double)n)) * diag[n - 1];
    // column c carries x/y terms of order m = c (c <= M) and z/w terms of order m = c - 1 (c - 1 <= M)
    n_cols = std::min(N + 1, M + 1);
    const double SQ2 = std::sqrt(2.0);
    ColHdr zero_hdr;
    std::memset(&zero_hdr, 0, sizeof zero_hdr);
    cols.assign(n_cols + 3, zero_hdr);  // spare tail entries: the kernel prefetches header c + 1
    col_len.assign(n_cols + 2, 0);
    tab.clear();
    for (int c = 1; c <= n_cols; ++c) {
        const int rows = N + 2 - c;
        const int nb = rows / HARM_BATCH, rem = rows % HARM_BATCH;  // full batches, then `rem` rows one at a time
        cols[c].start = (int32_t)tab.size();
        cols[c].nb = nb | (rem << 16);
        cols[c].rows = rows;
        cols[c].scale = (double)c * SQ2;
        cols[c].diag = diag[c];
        col_len[c] = rows;
        double B = 1.0;  // prod of b[k][c], k = c+1 .. n: the scale of the carried recursion variable (see HarmEntry)
        for (int n = c; n <= N + 1; ++n) {
            HarmEntry e;
            if (n == c) {
                e.g = -1.0;
            } else if (n == c + 1) {
                e.g = 0.0;
                B *= bnm(n, c);
            } else {
                e.g = cnm(n, c) / (bnm(n, c) * bnm(n - 1, c));
                B *= bnm(n, c);
            }
            e.t1 = B * C(n, c);
            e.t2 = B * S(n, c);
            // z: (n, m = c-1), n in 1..N
            const bool zok = (n >= 1 && n <= N);
            e.t3 = zok ? B * (SQ2 * vr01(n, c - 1) * C(n, c - 1)) : 0.0;
            e.t4 = zok ? B * (SQ2 * vr01(n, c - 1) * S(n, c - 1)) : 0.0;
            // w: (n-1, m = c-1), n-1 in 1..N
            const bool wok = (n - 1 >= 1 && n - 1 <= N && n - 1 >= c - 1);
            e.t5 = wok ? B * (SQ2 * vr11(n - 1, c - 1) * C(n - 1, c - 1)) : 0.0;
            e.t6 = wok ? B * (SQ2 * vr11(n - 1, c - 1) * S(n - 1, c - 1)) : 0.0;
            tab.push_back(e);
        }
    }
}

// The same table as ONE stream for the hybrid feed (devcfg.h, HYB_*): stream row r = entry r of `tab` (the columns' rows back to
// back).  Scalar side: {g, t1, t2}, 24 bytes per row; vector side, behind it: groups of sixteen rows, [t3..t6][16].
inline void build_hybrid(const std::vector<HarmEntry> &tab, std::vector<double> &hyb, int64_t &vec_off) {
    // whole groups, plus two more: the walk fetches one batch / one group past its last row
    const size_t n = tab.size(), padded = (n + 15) / 16 * 16 + 2 * 16;
    const HarmEntry z = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    hyb.clear();
    for (size_t r = 0; r < padded; ++r) {
        const HarmEntry &e = r < n ? tab[r] : z;
        hyb.push_back(e.g); hyb.push_back(e.t1); hyb.push_back(e.t2);
    }
    vec_off = (int64_t)hyb.size();  // 3 * padded doubles = a multiple of 48: the vector side starts 128-byte aligned
    for (size_t g = 0; g < padded / 16; ++g)
        for (int j = 0; j < 4; ++j)
            for (int l = 0; l < 16; ++l) {
                const size_t r = g * 16 + l;
                const HarmEntry &e = r < n ? tab[r] : z;
                hyb.push_back(j == 0 ? e.t3 : j == 1 ? e.t4 : j == 2 ? e.t5 : e.t6);
            }
}

// A run stream (DevCfg.rs_*): the rows of the schedules `ids` of `sched` (DevCfg.sched), every range of every wave laid out as one
// contiguous piece that starts a sixteen-row group of its own - a wave's walk then begins on its range's first row (in the common
// stream it begins at the batch that holds it, with up to seven rows of the previous column in front, through the recursion with a
// zero state: at 70x70 3 % of an owner's rows, and most of a short range).  `cols` / `tab`: the column headers and the entry table
// (without its tail padding); `cols_x` = the column headers with `start` pointing into this stream.
// Same rows, same operations: bit-identical sums.
inline void build_run_stream(const std::vector<ColHdr> &cols, const std::vector<HarmEntry> &tab, const DevSched *sched, std::initializer_list<int> ids,
                             std::vector<double> &hyb, int64_t &vec_off, std::vector<ColHdr> &cols_x) {
    cols_x = cols;
    std::vector<HarmEntry> t;
    const HarmEntry z = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    std::vector<char> seen(cols_x.size(), 0);
    for (int k : ids) {
        const DevSched &sd = sched[k];
        for (int w = 0; w < DEV_MAX_WAVES; ++w)
            for (int r = 0; r < sd.n_ranges[w]; ++r) {
                t.resize((t.size() + 15) / 16 * 16, z);
                for (int c = sd.range_c0[w][r]; c < sd.range_c0[w][r] + sd.range_cnt[w][r]; ++c) {
                    if (c < 1 || c >= (int)cols_x.size() || seen[c]) continue;
                    seen[c] = 1;
                    const int32_t src = cols[c].start;
                    cols_x[c].start = (int32_t)t.size();
                    for (int q = 0; q < cols[c].rows; ++q) t.push_back(tab[(size_t)src + q]);
                }
            }
    }
    build_hybrid(t, hyb, vec_off);
}

// What build_context hands nyx_hip_ctx_create: rc != NYX_HIP_RC_OK and `error`, or everything below.
struct CtxBuild {
    int rc = NYX_HIP_RC_OK;
    std::string error;
    DevCfg dc;                      // force-model part; no schedule yet, harm_feed = 0 (plan_first_schedule sets it)
    std::vector<double> records;    // device layout of the ephemeris records, 16 doubles of tail padding
    std::vector<HarmEntry> tab, tab2;  // harmonics tables of the two fields (without their tail padding)
    std::vector<ColHdr> cols, cols2;
    std::vector<int32_t> col_len;   // rows per column of the first field (index = c)
    int terms2 = 0;                 // table rows of the second field
    double role_handicap[3] = {0.0, 0.0, 0.0};  // integrator, almanac, perturbations (harmonics-term units)
    int ed_reuse_fit = 0;           // fields of stage-0 epoch data an unchained pipelined loop may carry between attempts (LDS room)
    int harm_feed = 0;              // DevCfg.harm_feed once the first schedule is built
    int swap_n_chain = 0;           // opts.integration_frame: the chain of state_frame_body w.r.t. the integration centre
    int32_t swap_seg[4] = {0, 0, 0, 0};
    double swap_sign[4] = {0.0, 0.0, 0.0, 0.0};

    CtxBuild() { std::memset(&dc, 0, sizeof dc); }
    int fail(int code, const char *fmt, ...) {
        char msg[512];
        va_list ap;
        va_start(ap, fmt); vsnprintf(msg, sizeof msg, fmt, ap); va_end(ap);
        error = msg;
        return rc = code;
    }
};

// A slot's chain stays in the configuration's segments (a body's, or an offset field's; an error otherwise).
inline bool chain_in_segments(const DevSlot &s, int n_seg) {
    for (int k = 0; k < s.n_chain; ++k) if (s.seg[k] < 0 || s.seg[k] >= n_seg) return false;
    return true;
}

// config + resolved tuning -> `b` (a fresh CtxBuild); returns b.rc.  The checks run in the order nyx_hip_ctx_create has always run
// them: a configuration with one error is told the same error.
inline int build_context(const nyx_hip_config_t &cfg, const nyx_hip_tuning_t &tune, LdsBytesFn lds_bytes, CtxBuild &b) {
    const nyx_hip_integ_opts_t &o = cfg.opts;
    const bool stm = (cfg.flags & NYX_HIP_FLAG_STM) != 0;
    if (o.method < 0 || o.method > 5 || o.error_ctrl < 0 || o.error_ctrl > 6) return b.fail(NYX_HIP_RC_BAD_ARG, "bad method / error_ctrl");
    if (stm && o.error_ctrl != NYX_HIP_RSS_CARTESIAN_STEP && o.error_ctrl != NYX_HIP_RSS_CARTESIAN_STATE)
        return b.fail(NYX_HIP_RC_UNSUPPORTED, "STM propagation on the device supports the RSSCartesianStep / RSSCartesianState error controls only");
    if ((cfg.flags & NYX_HIP_FLAG_STM_TEXTBOOK) && !stm) return b.fail(NYX_HIP_RC_BAD_ARG, "NYX_HIP_FLAG_STM_TEXTBOOK without NYX_HIP_FLAG_STM");
    if (cfg.drag && stm)  // PartialsUndefined in the reference too (drag.rs:286-294)
        return b.fail(NYX_HIP_RC_UNSUPPORTED, "drag has no partials: STM propagation with drag is undefined");
    if (cfg.drag && cfg.gravity && std::memcmp(&cfg.drag->rotation, &cfg.gravity->rotation, sizeof(nyx_hip_rotation_t)) != 0)
        return b.fail(NYX_HIP_RC_UNSUPPORTED, "device path: the drag frame must be the gravity-field frame when both are present");
    if (cfg.tides) {
        const nyx_hip_rotation_t *other = cfg.gravity ? &cfg.gravity->rotation : (cfg.drag ? &cfg.drag->rotation : nullptr);
        if (other && std::memcmp(&cfg.tides->rotation, other, sizeof(nyx_hip_rotation_t)) != 0)
            return b.fail(NYX_HIP_RC_UNSUPPORTED, "device path: the tidal frame must be the gravity-field / drag frame when they are present");
        if (cfg.tides->n_perturbers < 0 || cfg.tides->n_perturbers > NYX_HIP_MAX_BODIES || !(cfg.tides->mu_km3_s2 > 0.0) ||
            !(cfg.tides->eq_radius_km > 0.0))
            return b.fail(NYX_HIP_RC_BAD_ARG, "bad solid-tides model");
    }
    // ---- plain-data validation: nothing below may index past what the device code assumes
    if (cfg.n_bodies < 0 || cfg.n_bodies > NYX_HIP_MAX_BODIES || (cfg.n_bodies > 0 && !cfg.bodies) || cfg.n_segments < 0 ||
        (cfg.n_segments > 0 && !cfg.segments) || cfg.n_point_masses < 0 || cfg.n_point_masses > NYX_HIP_MAX_BODIES)
        return b.fail(NYX_HIP_RC_BAD_ARG, "bad body / segment / point-mass counts");
    for (int k = 0; k < cfg.n_bodies; ++k)
        if (cfg.bodies[k].n_chain < 0 || cfg.bodies[k].n_chain > NYX_HIP_MAX_CHAIN)
            return b.fail(NYX_HIP_RC_BAD_ARG, "body %d: n_chain %d outside 0..%d", k, cfg.bodies[k].n_chain, NYX_HIP_MAX_CHAIN);
    for (int i = 0; i < cfg.n_segments; ++i) {
        const nyx_hip_cheby_segment_t &sg = cfg.segments[i];
        if (sg.n_coeffs < 1 || sg.n_records < 1 || !(sg.interval_s > 0.0) || !sg.records)
            return b.fail(NYX_HIP_RC_BAD_ARG, "segment %d: n_coeffs >= 1, n_records >= 1, interval_s > 0 and records are required", i);
        if (sg.n_coeffs > NYX_HIP_MAX_CHEBY_COEFFS)  // (cheby_eval: a 16-wide register window, a rolled loop up to this limit)
            return b.fail(NYX_HIP_RC_UNSUPPORTED, "segment %d: %d Chebyshev coefficients per component, the device path evaluates at most %d", i,
                          sg.n_coeffs, NYX_HIP_MAX_CHEBY_COEFFS);
    }
    for (const nyx_hip_rotation_t *r : {cfg.gravity ? &cfg.gravity->rotation : nullptr, cfg.drag ? &cfg.drag->rotation : nullptr,
                                        cfg.tides ? &cfg.tides->rotation : nullptr, cfg.gravity2 ? &cfg.gravity2->rotation : nullptr})
        if (r)
            if (const char *why = check_rotation(*r, cfg.n_segments)) return b.fail(NYX_HIP_RC_BAD_ARG, "body-fixed orientation: %s", why);
    if (const uint32_t retired = (uint32_t)tune.debug_flags & ~kLiveDebugFlags)
        return b.fail(NYX_HIP_RC_BAD_ARG, "tuning.debug_flags 0x%x: not a debug switch of this library (the A/B path it selected was retired)",
                      retired & (0u - retired));

    DevCfg &dc = b.dc;
    const NyxTableau &tb = NYX_TABLEAUX[o.method];
    dc.stages = tb.stages; dc.order = tb.order;
    dc.fixed_step = o.fixed_step; dc.error_ctrl = o.error_ctrl; dc.attempts = o.attempts; dc.flags = (int32_t)cfg.flags;
    dc.flags |= tune.debug_flags & 0xff00;  // timing-only switches
    dc.tol = o.tolerance;
    dc.init_step_ns = o.init_step_ns; dc.min_step_ns = o.min_step_ns; dc.max_step_ns = o.max_step_ns;
    dc.min_step_s = ns_to_seconds_host(o.min_step_ns);
    dc.max_step_s = ns_to_seconds_host(o.max_step_ns);
    dc.inv_order = 1.0 / (double)tb.order;
    dc.inv_order_m1 = 1.0 / (double)(tb.order - 1);
    {
        int a_idx = 0;
        dc.c[0] = 0.0;
        for (int i = 0; i < tb.stages - 1; ++i) {  // c_i = running sum of row i (reference instance.rs:379-387)
            double ci = 0.0;
            for (int j = 0; j <= i; ++j) { dc.a[a_idx] = tb.a[a_idx]; ci += tb.a[a_idx]; ++a_idx; }
            dc.c[i + 1] = ci;
        }
        for (int i = 0; i < tb.stages; ++i) { dc.b[i] = tb.b[i]; dc.bdiff[i] = tb.b[i] - tb.b[i + tb.stages]; }
    }
    dc.mu_central = cfg.central_mu_km3_s2;
    dc.g_slot = -1;

    // ---- bodies -> slots (every non-central body referenced by a model)
    std::vector<int> slot_of(cfg.n_bodies, -1);
    auto slot_for = [&](int k) -> int {
        if (k < 0 || k >= cfg.n_bodies) return -2;
        if (cfg.bodies[k].n_chain == 0) return -1;  // the integration centre
        if (slot_of[k] >= 0) return slot_of[k];
        if (dc.n_slots >= DEV_MAX_SLOTS) return -2;
        const nyx_hip_body_t &bd = cfg.bodies[k];
        DevSlot &s = dc.slot[dc.n_slots];
        s.mu = bd.mu_km3_s2; s.radius = bd.mean_radius_km; s.n_chain = bd.n_chain;
        for (int q = 0; q < bd.n_chain; ++q) { s.seg[q] = bd.chain_segment[q]; s.sign[q] = (double)bd.chain_sign[q]; }
        slot_of[k] = dc.n_slots++;
        return slot_of[k];
    };
    for (int k = 0; k < cfg.n_bodies; ++k)
        if (cfg.bodies[k].n_chain == 0) dc.central_radius = cfg.bodies[k].mean_radius_km;
    if (cfg.state_frame_body != 0) {  // opts.integration_frame: the body the states are centred on
        const int k = cfg.state_frame_body;
        if (k < 0 || k >= cfg.n_bodies || cfg.bodies[k].n_chain > 4) return b.fail(NYX_HIP_RC_BAD_ARG, "state_frame_body: not a body of this configuration");
        b.swap_n_chain = cfg.bodies[k].n_chain;
        for (int q = 0; q < b.swap_n_chain; ++q) {
            const int sgi = cfg.bodies[k].chain_segment[q];
            if (sgi < 0 || sgi >= cfg.n_segments) return b.fail(NYX_HIP_RC_BAD_ARG, "state_frame_body: bad chain segment index");
            b.swap_seg[q] = sgi;
            b.swap_sign[q] = (double)cfg.bodies[k].chain_sign[q];
        }
    }
    for (int k = 0; k < cfg.n_point_masses; ++k) {
        const int s = slot_for(cfg.point_mass_body[k]);
        if (s == -2) return b.fail(NYX_HIP_RC_BAD_ARG, "too many / invalid point-mass bodies");
        if (s == -1) continue;  // central body is skipped by PointMasses::eom (orbital.rs:219-222)
        dc.pm_slot[dc.n_pm++] = s;
    }
    if (cfg.srp) {
        dc.has_srp = 1;
        dc.srp_estimate = cfg.srp->estimate;
        dc.phi = cfg.srp->phi_w_m2;
        dc.c_m_s = cfg.speed_of_light_km_s * 1e3;
        const int s = slot_for(cfg.srp->sun_body);
        if (s < 0) return b.fail(NYX_HIP_RC_BAD_ARG, "SRP light source must be a non-central body with an ephemeris");
        dc.sun_slot = s;
        dc.n_shadow = cfg.srp->n_shadow_bodies;
        if (dc.n_shadow > DEV_MAX_SLOTS) return b.fail(NYX_HIP_RC_BAD_ARG, "too many shadow bodies");
        for (int k = 0; k < dc.n_shadow; ++k) {
            const int sb = slot_for(cfg.srp->shadow_body[k]);
            if (sb == -2) return b.fail(NYX_HIP_RC_BAD_ARG, "invalid shadow body");
            dc.shadow_slot[k] = sb;
        }
    }
    if (cfg.tides) {
        const nyx_hip_solid_tides_t *td = cfg.tides;
        dc.has_tides = 1;
        dc.t_k2_5 = td->k2 / (2.0 * 2.0 + 1.0);
        dc.t_k3_7 = td->k3 / (2.0 * 3.0 + 1.0);
        dc.t_mu = td->mu_km3_s2; dc.t_re = td->eq_radius_km;
        copy_rotation(dc.t_rot, td->rotation);
        for (int j = 0; j < td->n_perturbers; ++j) {
            const int k = td->perturber_body[j];
            const int sl = slot_for(k);
            if (sl < 0) return b.fail(NYX_HIP_RC_BAD_ARG, "tidal perturbers must be non-central bodies with an ephemeris (and fit the %d slots)", DEV_MAX_SLOTS);
            dc.t_slot[dc.t_n] = sl;
            dc.t_deg3[dc.t_n] = td->compute_degree_3[j] ? 1 : 0;
            dc.t_gm_ratio[dc.t_n] = cfg.bodies[k].mu_km3_s2 / td->mu_km3_s2;
            dc.t_n++;
        }
    }
    // ---- segments
    if (cfg.n_segments > DEV_MAX_SEG) return b.fail(NYX_HIP_RC_BAD_ARG, "too many ephemeris segments");
    dc.n_seg = cfg.n_segments;
    // Device layout of the records.  cheby_eval() works on a sixteen-coefficient register window and has to blank the entries past a
    // segment's own count (two v_cndmask per coefficient on the almanac wave, every stage).  When the whole table stays small the
    // records of segments with <= 16 coefficients are therefore laid out SIXTEEN wide, zero-padded: the zeros are in the table, the
    // selects go (DevSeg.stride = 50 tells the kernel; same values, same bits).
    const int kChebWin = 16;
    auto fits_lds = [&](int rec_doubles) {  // (rec_in_lds below: for this context's kernel family)
        return records_fit_lds(lds_bytes, rec_doubles, stm ? DEV_MAX_WAVES_STM : DEV_MAX_WAVES, stm ? 1 : 0, 0);
    };
    bool pad16 = true;
    {
        size_t packed = 0, padded = 0;
        for (int i = 0; i < cfg.n_segments; ++i) {
            const nyx_hip_cheby_segment_t &sg = cfg.segments[i];
            packed += (size_t)sg.n_records * (size_t)(2 + 3 * sg.n_coeffs);
            padded += (size_t)sg.n_records * (size_t)(2 + 3 * (sg.n_coeffs <= kChebWin ? kChebWin : sg.n_coeffs));
        }
        if (fits_lds((int)packed + 16) && !fits_lds((int)padded + 16)) pad16 = false;  // (never push the table out of LDS)
        if (padded * sizeof(double) > (size_t)8 << 20) pad16 = false;
    }
    std::vector<double> &records = b.records;
    for (int i = 0; i < cfg.n_segments; ++i) {
        const nyx_hip_cheby_segment_t &sg = cfg.segments[i];
        DevSeg &d = dc.seg[i];
        d.init_et = sg.init_et_s; d.interval = sg.interval_s; d.n_rec = sg.n_records; d.n_coef = sg.n_coeffs;
        d.end_et = sg.init_et_s + sg.interval_s * (double)sg.n_records;
        const int src_stride = 2 + 3 * sg.n_coeffs;
        d.offset = (int32_t)records.size();
        if (pad16 && sg.n_coeffs < kChebWin) {
            d.stride = 2 + 3 * kChebWin;
            for (int r = 0; r < sg.n_records; ++r) {
                const double *src = sg.records + (size_t)r * src_stride;
                records.push_back(src[0]); records.push_back(src[1]);
                for (int c = 0; c < 3; ++c)
                    for (int j = 0; j < kChebWin; ++j) records.push_back(j < sg.n_coeffs ? src[2 + c * sg.n_coeffs + j] : 0.0);
            }
        } else {
            d.stride = src_stride;
            records.insert(records.end(), sg.records, sg.records + (size_t)sg.n_records * d.stride);
        }
    }
    for (int s = 0; s < dc.n_slots; ++s)
        if (!chain_in_segments(dc.slot[s], dc.n_seg)) return b.fail(NYX_HIP_RC_BAD_ARG, "bad chain segment index");

    // ---- gravity fields.  The field of another body than the integration centre (gravity_field.rs:150-154) names it in offset_body:
    // its slot (-1: the integration centre itself); false once b.fail() has been told why not.
    auto offset_slot = [&](const nyx_hip_gravity_field_t *g, const char *what, int32_t &slot) {
        slot = g->offset_body == 0 ? -1 : slot_for(g->offset_body - 1);
        if (slot == -2) b.fail(NYX_HIP_RC_BAD_ARG, "%s: offset_body is not a body of this configuration (or the %d body slots are taken)", what, DEV_MAX_SLOTS);
        else if (slot >= 0 && !chain_in_segments(dc.slot[slot], dc.n_seg)) b.fail(NYX_HIP_RC_BAD_ARG, "bad chain segment index");
        return b.rc == NYX_HIP_RC_OK;
    };
    if (cfg.gravity) {
        const nyx_hip_gravity_field_t *g = cfg.gravity;
        if (g->degree < 1 || !g->c_nm || !g->s_nm) return b.fail(NYX_HIP_RC_BAD_ARG, "bad gravity field");
        dc.has_grav = 1; dc.deg = g->degree; dc.ord = std::min(g->order, g->degree);
        if (!offset_slot(g, "gravity field", dc.g_slot)) return b.rc;
        dc.g_mu = g->mu_km3_s2; dc.g_re = g->eq_radius_km; dc.g_inv_re = 1.0 / g->eq_radius_km;
        copy_rotation(dc.g_rot, g->rotation);
        int n_cols = 0;
        build_harmonics(g, b.tab, b.cols, b.col_len, n_cols);
        dc.n_cols = n_cols;
    }
    if (cfg.gravity2) {
        const nyx_hip_gravity_field_t *g = cfg.gravity2;
        if (!cfg.gravity) return b.fail(NYX_HIP_RC_BAD_ARG, "gravity2 without gravity: a single field goes into `gravity`");
        if (g->degree < 1 || !g->c_nm || !g->s_nm) return b.fail(NYX_HIP_RC_BAD_ARG, "bad second gravity field");
        dc.has_grav2 = 1;
        dc.g2_mu = g->mu_km3_s2; dc.g2_re = g->eq_radius_km; dc.g2_inv_re = 1.0 / g->eq_radius_km;
        copy_rotation(dc.g2_rot, g->rotation);
        if (!offset_slot(g, "second gravity field", dc.g2_slot)) return b.rc;
        std::vector<int32_t> len2;
        int n_cols2 = 0;
        build_harmonics(g, b.tab2, b.cols2, len2, n_cols2);
        dc.n_cols2 = n_cols2;
        for (int32_t l : len2) b.terms2 += l;
    }
    if (cfg.drag) {
        const nyx_hip_drag_t *dg = cfg.drag;
        if (dg->density < 0 || dg->density > 2) return b.fail(NYX_HIP_RC_BAD_ARG, "bad drag density model");
        dc.has_drag = 1; dc.drag_density = dg->density;
        dc.drag_rho0 = dg->rho0; dc.drag_r0 = dg->r0; dc.drag_ref_alt_m = dg->ref_alt_m; dc.drag_max_alt_m = dg->max_alt_m;
        dc.drag_re = dg->eq_radius_km;
        copy_rotation(dc.d_rot, dg->rotation);
    }
    // serial duties of the role waves per force evaluation, in units of one harmonics term (~10 f64 ops):
    // integrator: stage combination, body-fixed transform, fold of the partials; almanac: 3 sincos + Chebyshev
    // chains; perturbations: third-body and SRP/eclipse terms.
    {
        int nseg_eval = 0;
        for (int s = 0; s < dc.n_slots; ++s) nseg_eval += dc.slot[s].n_chain;
        // (refitted in round 3 to the duties the calibration measures on the BASELINE workloads: 70x70 + Sun / Moon + SRP gives
        //  integrator 66, almanac 140, perturbations 52 harmonics-term units - the first formulas were 2.2x too low)
        b.role_handicap[0] = 60.0;
        b.role_handicap[1] = 26.0 * nseg_eval + (dc.has_grav ? 38.0 : 0.0);
        b.role_handicap[2] = (dc.has_grav2 ? 38.0 + 1.1 * b.terms2 : 0.0) + 13.0 * dc.n_pm + (dc.has_srp ? 13.0 + 13.0 * dc.n_shadow : 0.0) +
                             (dc.has_drag ? 22.0 : 0.0) + (dc.has_tides ? 30.0 + 17.0 * dc.t_n : 0.0);
        if (has_nonzero(tune.role_duties, 3))
            for (int k = 0; k < 3; ++k) b.role_handicap[k] = tune.role_duties[k];
    }
    {
        // the body-fixed frame of the epoch data (the kernel's choice: gravity field, else drag, else tides): a polynomial IAU
        // orientation is advanced from a base epoch instead of being evaluated with three full-range sincos per stage
        const DevRot &er = dc.has_grav ? dc.g_rot : (dc.has_drag ? dc.d_rot : dc.t_rot);
        // (plain kernels only: the STM tests hold the device to the oracle's step sequence, bit for bit)
        dc.dcm_incr = ((dc.has_grav || dc.has_drag || dc.has_tides) && er.kind == NYX_HIP_ROT_IAU && er.n_np == 0 && !stm &&
                       !(tune.debug_flags & 0x4000)) ? 1 : 0;
    }
    records.resize(records.size() + 16, 0.0);  // padding for the 16-wide coefficient window
    dc.rec_doubles = (int32_t)records.size();
    dc.rec_in_lds = fits_lds(dc.rec_doubles) ? 1 : 0;
    // stage-0 epoch data carried between attempts (see role_loop): needs an even stage count (the last stage's window
    // then leaves buffer 0 free) and 9 + 3 * n_slots doubles + 20 bytes of LDS per lane
    dc.ed_reuse = 0;
    if (!stm && dc.stages % 2 == 0 && tune.epoch_data_reuse != 0) {
        const int nf = 9 + 3 * dc.n_slots;
        if (lds_bytes(DEV_MAX_WAVES, dc.rec_in_lds ? dc.rec_doubles : 0, 0, nf) <= kKernelLdsMax) dc.ed_reuse = nf;
    }
    b.ed_reuse_fit = dc.ed_reuse;
    dc.coop_frac = 0.30;  // measured optimum with two owners per helper (10 000 trajectories, 70x70): 0.28-0.33 is flat
    if (tune.coop_fraction > 0.0) dc.coop_frac = std::min(0.9, std::max(0.05, tune.coop_fraction));
    if (!b.tab.empty()) {
        // measured (same box, calibrated): 150x150 cooperative 373 -> 334 ms per 6 250 x 3 h (1.12x); 70x70 alone 1.02-1.11x;
        // 70x70 cooperative (one column per helper wave and job: the walk's start-up weighs more) 0-2 % slower
        // (DevCfg.harm_feed: bit 0 = the trajectory-owning workgroups, bit 1 = the helpers and the owner's fallback for them)
        // Round 4: the trajectory-owning workgroups stream the table from degree 40 on (with ONE contiguous run of columns per wave,
        // fill_schedule: the start-up of a run is what the walk costs at 70x70), the helpers - one column per wave and job - above 95
        b.harm_feed = dc.n_cols > 96 ? 3 : (dc.n_cols > 40 ? 1 : 0);
        if (tune.harmonics_feed >= 0) b.harm_feed = tune.harmonics_feed == 0 ? 0 : (tune.harmonics_feed == 2 ? 1 : (tune.harmonics_feed == 3 ? 2 : 3));
    }
    return NYX_HIP_RC_OK;
}

// The first schedule of a new context: built with harm_feed = 0, the feed set after it.  The planner reads harm_feed, so this order
// fixes the first schedule, hence bits of every result.
inline void plan_first_schedule(const PlanInputs &in, DevCfg &dc, SchedShape &shape, int harm_feed) {
    dc.harm_feed = 0;
    build_schedule(in, dc, shape, 1);
    dc.harm_feed = harm_feed;
}
