// launch_plan_cases.h - the launch shapes tests/cxx/launch_plan_check.cpp plans (nyx_amd/csrc/launch_plan.h), and the one-line text
// form of a plan that tests/golden/launch_plans.txt holds.  Force-model part of the DevCfg of the BASELINE workloads, built by hand the
// way nyx_hip_ctx_create builds it (slots in the order the models name their bodies; the segments of nyx_amd/ephem.py:
// 0 Sun / SSB (11 coefficients), 1 EMB / SSB, 2 Earth / EMB, 3 Moon / EMB (13 each), 4 Jupiter barycentre / SSB (8)).
#pragma once
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../nyx_amd/csrc/devcfg.h"

namespace lpc {

struct Shape {
    std::string name;
    std::unique_ptr<DevCfg> dc;     // force-model part; harm_feed = 0, as when nyx_hip_ctx_create builds the first schedule
    int harm_feed = 0;              // set after that first schedule (nyx_hip_ctx_create)
    std::vector<int32_t> col_len;
    int terms2 = 0;
};

struct Variant {
    std::string name;
    nyx_hip_tuning_t tune;
    bool inject_weights = false;    // a calibrated-weights entry for every workgroup shape
};

inline void add_slot(DevCfg &dc, std::initializer_list<int> segs) {
    DevSlot &s = dc.slot[dc.n_slots++];
    s.n_chain = 0;
    for (int g : segs) s.seg[s.n_chain++] = g;
}

inline void add_field(DevCfg &dc, std::vector<int32_t> &col_len, int deg) {
    dc.has_grav = 1; dc.deg = deg; dc.ord = deg; dc.n_cols = deg + 1;
    col_len.assign(dc.n_cols + 2, 0);
    for (int c = 1; c <= dc.n_cols; ++c) col_len[c] = deg + 2 - c;  // (build_harmonics: rows of column c)
}

// what nyx_hip_ctx_create derives: the harmonics feed by field size, the role duties
inline int auto_harm_feed(const DevCfg &dc) { return dc.n_cols > 96 ? 3 : (dc.n_cols > 40 ? 1 : 0); }

inline std::vector<Shape> shapes() {
    std::vector<Shape> v;
    auto mk = [&](const char *name, int stages, uint32_t flags) -> Shape & {
        v.emplace_back();
        Shape &s = v.back();
        s.name = name;
        s.dc.reset(new DevCfg);
        std::memset(s.dc.get(), 0, sizeof(DevCfg));
        s.dc->stages = stages; s.dc->flags = (int32_t)flags; s.dc->g_slot = -1; s.dc->g2_slot = -1;
        s.dc->n_seg = 5;
        const int coef[5] = {11, 13, 13, 13, 8};
        for (int k = 0; k < 5; ++k) s.dc->seg[k].n_coef = coef[k];
        return s;
    };
    auto earth_sun_moon = [](DevCfg &dc) {  // PointMasses(Sun, Moon) + SRP with the Earth's shadow
        add_slot(dc, {0, 1, 2}); add_slot(dc, {3, 2});
        dc.n_pm = 2; dc.pm_slot[0] = 0; dc.pm_slot[1] = 1;
        dc.has_srp = 1; dc.sun_slot = 0; dc.n_shadow = 1; dc.shadow_slot[0] = -1;
    };
    {   // configs[1] (bench --config 2): 70x70 + Sun / Moon + SRP, RK89
        Shape &s = mk("cfg2_70x70", 16, 0);
        earth_sun_moon(*s.dc); add_field(*s.dc, s.col_len, 70);
    }
    {   // config 3: JWST, Moon / Sun / Jupiter point masses + SRP (Earth and Moon shadows), no field
        Shape &s = mk("cfg3_jwst", 16, 0);
        add_slot(*s.dc, {3, 2}); add_slot(*s.dc, {0, 1, 2}); add_slot(*s.dc, {4, 1, 2});
        s.dc->n_pm = 3; for (int k = 0; k < 3; ++k) s.dc->pm_slot[k] = k;
        s.dc->has_srp = 1; s.dc->sun_slot = 1; s.dc->n_shadow = 2; s.dc->shadow_slot[0] = -1; s.dc->shadow_slot[1] = 0;
    }
    {   // config 4: STM on a 21x21 field + Sun / Moon + SRP (quad or D3 layout by ensemble size)
        Shape &s = mk("cfg4_stm21", 16, NYX_HIP_FLAG_STM);
        earth_sun_moon(*s.dc); add_field(*s.dc, s.col_len, 21);
    }
    {   // config 5: 150x150 lunar field + Earth / Sun point masses, DP78, Moon-centred chains
        Shape &s = mk("cfg5_150x150", 13, 0);
        add_slot(*s.dc, {2, 3}); add_slot(*s.dc, {0, 1, 3});
        s.dc->n_pm = 2; s.dc->pm_slot[0] = 0; s.dc->pm_slot[1] = 1;
        add_field(*s.dc, s.col_len, 150);
    }
    {   // a 21x21 field without the STM: eight-wave workgroups
        Shape &s = mk("deg21", 16, 0);
        earth_sun_moon(*s.dc); add_field(*s.dc, s.col_len, 21);
    }
    {   // a second field (a 10x10 lunar field beside the 70x70 Earth field)
        Shape &s = mk("grav2_70+10", 16, 0);
        earth_sun_moon(*s.dc); add_field(*s.dc, s.col_len, 70);
        s.dc->has_grav2 = 1; s.dc->n_cols2 = 11; s.dc->g2_slot = 1;
        for (int c = 1; c <= 11; ++c) s.terms2 += 12 - c;
    }
    for (Shape &s : v) s.harm_feed = auto_harm_feed(*s.dc);
    return v;
}

// nyx_hip_ctx_create: integrator, almanac, perturbation duties in harmonics-term units
inline void role_handicap(const DevCfg &dc, const nyx_hip_tuning_t &t, int terms2, double *rh) {
    int nseg_eval = 0;
    for (int s = 0; s < dc.n_slots; ++s) nseg_eval += dc.slot[s].n_chain;
    rh[0] = 60.0;
    rh[1] = 26.0 * nseg_eval + (dc.has_grav ? 38.0 : 0.0);
    rh[2] = (dc.has_grav2 ? 38.0 + 1.1 * terms2 : 0.0) + 13.0 * dc.n_pm + (dc.has_srp ? 13.0 + 13.0 * dc.n_shadow : 0.0) + (dc.has_drag ? 22.0 : 0.0) +
            (dc.has_tides ? 30.0 + 17.0 * dc.t_n : 0.0);
    if (t.role_duties[0] != 0.0 || t.role_duties[1] != 0.0 || t.role_duties[2] != 0.0)
        for (int k = 0; k < 3; ++k) rh[k] = t.role_duties[k];
}
// nyx_hip_ctx_create: the stage-0 epoch data an unchained loop may carry (the LDS always has room for the shapes here)
inline int ed_reuse_fit(const DevCfg &dc, const nyx_hip_tuning_t &t) {
    return (!(dc.flags & NYX_HIP_FLAG_STM) && dc.stages % 2 == 0 && t.epoch_data_reuse != 0) ? 9 + 3 * dc.n_slots : 0;
}
inline double initial_coop_frac(const nyx_hip_tuning_t &t) {
    return t.coop_fraction > 0.0 ? (t.coop_fraction < 0.05 ? 0.05 : (t.coop_fraction > 0.9 ? 0.9 : t.coop_fraction)) : 0.30;
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
