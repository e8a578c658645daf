// launch_plan_cases.h - the launch shapes tests/cxx/launch_plan_check.cpp plans (nyx_amd/csrc/launch_plan.h), and the one-line text
// form of a plan that tests/golden/launch_plans.txt holds.  The shapes are the configurations of the BASELINE workloads as
// nyx_hip_config_t, built into a DevCfg by nyx_amd/csrc/ctx_build.h as nyx_hip_ctx_create builds them.  Bodies with the chains of
// nyx_amd/ephem.py through its segments 0 Sun / SSB (11 coefficients), 1 EMB / SSB, 2 Earth / EMB, 3 Moon / EMB (13 each),
// 4 Jupiter barycentre / SSB (8); synthetic records and Stokes coefficients (a plan depends on their counts only).
#pragma once
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/nyx_hip.h"
#include "../../nyx_amd/csrc/devcfg.h"

namespace lpc {

// A nyx_hip_config_t and the storage it points into (not copyable: it points into itself).
struct Config {
    nyx_hip_config_t cfg{};
    nyx_hip_body_t bodies[NYX_HIP_MAX_BODIES]{};
    nyx_hip_cheby_segment_t segments[NYX_HIP_MAX_SEGMENTS]{};
    std::vector<double> records[NYX_HIP_MAX_SEGMENTS];
    nyx_hip_gravity_field_t field[2]{};
    std::vector<double> stokes[4];  // C, S of field[0], then of field[1]
    nyx_hip_srp_t srp{};
    nyx_hip_drag_t drag{};
    nyx_hip_solid_tides_t tides{};
    Config() = default;
    Config(const Config &) = delete;
    Config &operator=(const Config &) = delete;
};

// bodies of ephem_config(): Earth-centred (build_almanac) and Moon-centred (build_moon_centered_almanac)
enum { EARTH = 0, SUN = 1, MOON = 2, JUPITER = 3 };
enum { MC_MOON = 0, MC_EARTH = 1, MC_SUN = 2 };

inline void add_segment(Config &c, int n_coeffs, int n_records = 2) {
    const int i = c.cfg.n_segments++;
    std::vector<double> &r = c.records[i];
    r.resize((size_t)n_records * (2 + 3 * n_coeffs));
    for (size_t k = 0; k < r.size(); ++k) r[k] = 1e3 * (i + 1) / (1.0 + (double)k) - 7.0 * (double)(k % 5);
    c.segments[i] = nyx_hip_cheby_segment_t{7.6e8, 16 * 86400.0, n_records, n_coeffs, r.data()};
}

inline void add_body(Config &c, double mu, double radius, std::initializer_list<int> chain, std::initializer_list<int> signs) {
    nyx_hip_body_t &b = c.bodies[c.cfg.n_bodies++];
    b.naif_id = 10 * c.cfg.n_bodies;
    b.mu_km3_s2 = mu; b.mean_radius_km = radius;
    for (int g : chain) b.chain_segment[b.n_chain++] = g;
    int k = 0;
    for (int s : signs) b.chain_sign[k++] = s;
}

inline nyx_hip_rotation_t iau_rotation(int n_nut_prec = 0) {  // an IAU orientation (Earth-like), optionally with nutation terms
    nyx_hip_rotation_t r{};
    r.kind = NYX_HIP_ROT_IAU;
    r.ra_deg[1] = -0.641; r.dec_deg[0] = 90.0; r.dec_deg[1] = -0.557; r.w_deg[0] = 190.147; r.w_deg[1] = 360.9856235;
    r.n_nut_prec = n_nut_prec;
    for (int k = 0; k < n_nut_prec; ++k) { r.nut_prec_angle_deg[k][0] = 125.0 + k; r.nut_prec_angle_deg[k][1] = -0.05 * (k + 1); r.nut_prec_ra[k] = 1e-3 * (k + 1); }
    return r;
}

// field k (0: config.gravity, 1: config.gravity2): degree x degree, synthetic Stokes coefficients
inline void set_field(Config &c, int k, int degree, int offset_body = 0) {
    nyx_hip_gravity_field_t &f = c.field[k];
    const size_t n = (size_t)(degree + 1) * (degree + 2) / 2;
    std::vector<double> &C = c.stokes[2 * k], &S = c.stokes[2 * k + 1];
    C.resize(n); S.resize(n);
    for (size_t q = 0; q < n; ++q) { C[q] = q == 0 ? 1.0 : 1e-6 / (1.0 + (double)q); S[q] = q % 3 ? -5e-7 / (2.0 + (double)q) : 0.0; }
    f.degree = degree; f.order = degree; f.offset_body = offset_body;
    f.mu_km3_s2 = k ? 4902.8 : 398600.4415; f.eq_radius_km = k ? 1738.0 : 6378.1363;
    f.c_nm = C.data(); f.s_nm = S.data();
    f.rotation = iau_rotation();
    (k ? c.cfg.gravity2 : c.cfg.gravity) = &f;
}

// the five segments and the bodies of one almanac; integration options of the BASELINE runs
inline std::unique_ptr<Config> ephem_config(int method, uint32_t flags, bool moon_centred = false) {
    std::unique_ptr<Config> p(new Config);
    Config &c = *p;
    c.cfg.abi_version = NYX_HIP_ABI_VERSION;
    c.cfg.flags = flags;
    c.cfg.opts = nyx_hip_integ_opts_t{60000000000LL, 1000000LL, 2700000000000LL, 1e-12, 50, 0, NYX_HIP_RSS_CARTESIAN_STEP, method};
    c.cfg.speed_of_light_km_s = 299792.458;
    c.cfg.segments = c.segments;
    c.cfg.bodies = c.bodies;
    for (int n : {11, 13, 13, 13, 8}) add_segment(c, n);
    if (moon_centred) {
        c.cfg.central_mu_km3_s2 = 4902.8;
        add_body(c, 4902.8, 1737.4, {}, {});
        add_body(c, 398600.4415, 6378.1363, {2, 3}, {+1, -1});
        add_body(c, 1.32712440018e11, 695700.0, {0, 1, 3}, {+1, -1, -1});
    } else {
        c.cfg.central_mu_km3_s2 = 398600.4415;
        add_body(c, 398600.4415, 6378.1363, {}, {});
        add_body(c, 1.32712440018e11, 695700.0, {0, 1, 2}, {+1, -1, -1});
        add_body(c, 4902.8, 1737.4, {3, 2}, {+1, -1});
        add_body(c, 1.26712764e8, 71492.0, {4, 1, 2}, {+1, -1, -1});
    }
    return p;
}

inline void point_masses(Config &c, std::initializer_list<int> bodies) { for (int b : bodies) c.cfg.point_mass_body[c.cfg.n_point_masses++] = b; }

inline void add_srp(Config &c, int sun, std::initializer_list<int> shadows) {
    c.srp.phi_w_m2 = 1367.0; c.srp.sun_body = sun;
    for (int b : shadows) c.srp.shadow_body[c.srp.n_shadow_bodies++] = b;
    c.cfg.srp = &c.srp;
}

// configs[1]'s force model (bench --config 2) on a degree x degree field: Sun / Moon point masses + SRP with the Earth's shadow, RK89
inline std::unique_ptr<Config> earth_sun_moon(int degree, uint32_t flags = 0) {
    std::unique_ptr<Config> p = ephem_config(NYX_HIP_RK89, flags);
    point_masses(*p, {SUN, MOON});
    add_srp(*p, SUN, {EARTH});
    set_field(*p, 0, degree);
    return p;
}

struct Shape {
    std::string name;
    std::unique_ptr<Config> cfg;
};

struct Variant {
    std::string name;
    nyx_hip_tuning_t tune;
    bool inject_weights = false;    // a calibrated-weights entry for every workgroup shape
};

// the LDS of the shapes here always has room for their records and the carried epoch data
inline size_t lds_room(int, int, int, int) { return 0; }

inline std::vector<Shape> shapes() {
    std::vector<Shape> v;
    // configs[1] (bench --config 2): 70x70 + Sun / Moon + SRP, RK89
    v.push_back(Shape{"cfg2_70x70", earth_sun_moon(70)});
    {   // config 3: JWST, Moon / Sun / Jupiter point masses + SRP (Earth and Moon shadows), no field
        std::unique_ptr<Config> p = ephem_config(NYX_HIP_RK89, 0);
        point_masses(*p, {MOON, SUN, JUPITER});
        add_srp(*p, SUN, {EARTH, MOON});
        v.push_back(Shape{"cfg3_jwst", std::move(p)});
    }
    // config 4: STM on a 21x21 field + Sun / Moon + SRP (quad or D3 layout by ensemble size)
    v.push_back(Shape{"cfg4_stm21", earth_sun_moon(21, NYX_HIP_FLAG_STM)});
    {   // config 5: 150x150 lunar field + Earth / Sun point masses, DP78, Moon-centred chains
        std::unique_ptr<Config> p = ephem_config(NYX_HIP_DP78, 0, true);
        point_masses(*p, {MC_EARTH, MC_SUN});
        set_field(*p, 0, 150);
        v.push_back(Shape{"cfg5_150x150", std::move(p)});
    }
    // a 21x21 field without the STM: eight-wave workgroups
    v.push_back(Shape{"deg21", earth_sun_moon(21)});
    {   // a second field (a 10x10 lunar field beside the 70x70 Earth field)
        std::unique_ptr<Config> p = earth_sun_moon(70);
        set_field(*p, 1, 10, MOON + 1);
        v.push_back(Shape{"grav2_70+10", std::move(p)});
    }
    return v;
}

inline std::vector<Variant> variants() {
    std::vector<Variant> v;
    auto add = [&](const char *name) -> nyx_hip_tuning_t & {
        v.push_back(Variant{name, NYX_HIP_TUNING_DEFAULT, false});
        return v.back().tune;
    };
    add("default");
    add("dbg0x8000").debug_flags = 0x8000;
    add("dbg0x10000").debug_flags = 0x10000;
    add("dbg0x2000000").debug_flags = 0x2000000;
    add("dbg0x80000").debug_flags = 0x80000;
    add("dbg0x8000000").debug_flags = 0x8000000;
    add("coop0").cooperative = 0;
    add("determ").deterministic = 1;
    add("frac0.33").coop_fraction = 0.33;
    add("frac0.36+dbg0x2000000").coop_fraction = 0.36;
    v.back().tune.debug_flags = 0x2000000;
    add("maxcols20").coop_max_columns = 20;
    add("maxcols6").coop_max_columns = 6;
    {
        nyx_hip_tuning_t &t = add("explicit");
        t.schedule = NYX_HIP_SCHED_EXPLICIT;
        const double w[16] = {1.0, 1.2, 0.7, 1.7, 1.9, 1.3, 1.5, 1.1, 1.0, 0.9, 0.8, 0.7, 0.5, 0.4, 0.3, 0.2};
        for (int k = 0; k < 16; ++k) t.wave_weights[k] = w[k];
    }
    {
        nyx_hip_tuning_t &t = add("duties+pipe0");
        t.pipelined = 0;
        t.role_duties[0] = 60.0; t.role_duties[1] = 600.0; t.role_duties[2] = 52.0;
    }
    add("pipe0").pipelined = 0;
    add("helpers1.5").coop_helper_ratio = 1.5;
    add("calibrated");
    v.back().inject_weights = true;
    return v;
}

// the injected calibrated entry: speed weights and duties of a made-up calibration, for every key a launch can ask for
template <typename Map> void inject_weights(Map &m) {
    typename Map::mapped_type a;
    for (int w = 0; w < DEV_MAX_WAVES; ++w) {
        a[w] = 1.5 - w / 16.0 + (w % 4 == 1 ? 0.25 : 0.0);
        a[DEV_MAX_WAVES + w] = w < 3 ? 40.0 + 10.0 * w : 0.0;
    }
    for (int nw : {1, 3, 4, 8, 16})
        for (int pipe = 0; pipe < 2; ++pipe)
            for (int quad = 0; quad < 2; ++quad)
                for (int tenths = -1; tenths <= 9; ++tenths) m[typename Map::key_type(nw, pipe, quad, tenths)] = a;
}

static const int64_t kSizes[] = {64, 640, 1250, 2500, 5000, 6250, 10000, 16384};
static const int64_t kSequence[] = {1280, 10000, 1280, 640, 5000, 16384, 64};  // one context, launch after launch

// One plan as a line of text: the launch shape, every schedule (wave:first+count ranges), the roles, the stage-loop switches and the
// cooperative mode of the launch (helpers/base/parts/fan, or - when the workgroups work alone).
inline std::string plan_line(const std::string &tag, const DevCfg &dc, int nw, bool quad, bool coop, int64_t helpers, int64_t base, int parts, bool fan) {
    std::string s = tag;
    char b[96];
    std::snprintf(b, sizeof b, " nw=%d quad=%d", nw, quad ? 1 : 0); s += b;
    std::snprintf(b, sizeof b, " pipe=%d spec=%d ed_reuse=%d seg_mode=%d n_alm=%d offload=%d qpre_off=%d merge=%d", dc.pipe, dc.spec, dc.ed_reuse,
                  dc.seg_mode, dc.n_alm, dc.offload, dc.qpre_off, dc.merge_roles); s += b;
    if (dc.seg_mode) {
        std::snprintf(b, sizeof b, " useg=%d@%d:", dc.n_useg, dc.ed_seg_base); s += b;
        for (int u = 0; u < dc.n_useg; ++u) { std::snprintf(b, sizeof b, "%d,", dc.useg_seg[u]); s += b; }
    }
    std::snprintf(b, sizeof b, " coop_ok=%d frac=%.17g", dc.coop_ok, dc.coop_frac); s += b;
    if (coop) { std::snprintf(b, sizeof b, " coop=%lld/%lld/%d/%d", (long long)helpers, (long long)base, parts, fan ? 1 : 0); s += b; }
    else s += " coop=-";
    s += " roles=";
    for (int w = 0; w < DEV_MAX_WAVES; ++w) { std::snprintf(b, sizeof b, "%d.%x.%d,", dc.role_kind[w], dc.role_mask[w], dc.role_slot[w]); s += b; }
    for (int k = 0; k < DEV_N_SCHED; ++k) {
        const DevSched &sd = dc.sched[k];
        bool any = false;
        for (int w = 0; w < DEV_MAX_WAVES; ++w) any = any || sd.n_ranges[w] != 0;
        if (!any) continue;
        std::snprintf(b, sizeof b, " s%d:", k); s += b;
        for (int w = 0; w < DEV_MAX_WAVES; ++w) {
            if (!sd.n_ranges[w]) continue;
            std::snprintf(b, sizeof b, "%d=", w); s += b;
            for (int r = 0; r < sd.n_ranges[w]; ++r) { std::snprintf(b, sizeof b, "%s%d+%d", r ? "," : "", sd.range_c0[w][r], sd.range_cnt[w][r]); s += b; }
            s += "/";
        }
    }
    return s;
}

}  // namespace lpc
