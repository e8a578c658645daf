// Stand-alone check of the context builder (nyx_amd/csrc/ctx_build.h) - g++ only, no HIP, no GPU (tests/test_ctx_build.py).
//   ctx_build_check OUT
// builds every case below under three LDS fakes, plans the first schedule on a 256-CU device and writes one line per case and fake
// to OUT: the rc and message of a refusal, or FNV-1a digests of everything a context starts with (compared with
// tests/golden/ctx_build.txt by the test).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../nyx_amd/csrc/ctx_build.h"
#include "launch_plan_cases.h"

namespace cbc {

using lpc::Config;

inline size_t lds_none(int, int, int, int) { return kKernelLdsMax + 1; }
inline size_t lds_tight(int, int rec_doubles, int, int) { return rec_doubles <= 400 ? 0 : kKernelLdsMax + 1; }  // (configs[1]: packed fits, padded not)
struct Fake { const char *name; LdsBytesFn fn; };
static const Fake kFakes[] = {{"room", lpc::lds_room}, {"tight", lds_tight}, {"none", lds_none}};

struct Case {
    std::string name;
    std::unique_ptr<Config> cfg;
    nyx_hip_tuning_t tune;
};

// What a context starts with: the builder's output, the first schedule planned into the DevCfg, the hybrid-feed stream.
struct Result {
    int rc = NYX_HIP_RC_OK;
    std::string error;
    std::unique_ptr<DevCfg> dc{new DevCfg()};
    std::vector<double> records, hyb;
    std::vector<HarmEntry> tab, tab2;
    std::vector<ColHdr> cols, cols2;
    std::vector<int32_t> col_len;
    double rh[3] = {0.0, 0.0, 0.0};
    int ed_reuse_fit = 0, terms2 = 0, swap_n_chain = 0;
    int32_t swap_seg[4] = {0, 0, 0, 0};
    double swap_sign[4] = {0.0, 0.0, 0.0, 0.0};
};

inline uint64_t fnv1a(const void *p, size_t n) {
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t k = 0; k < n; ++k) { h ^= ((const unsigned char *)p)[k]; h *= 0x100000001b3ull; }
    return h;
}
template <typename T> uint64_t digest(const std::vector<T> &v) { return fnv1a(v.data(), v.size() * sizeof(T)); }

inline std::string result_line(const std::string &tag, const Result &r) {
    char b[1024];
    if (r.rc != NYX_HIP_RC_OK) {
        std::snprintf(b, sizeof b, "%s rc=%d %s", tag.c_str(), r.rc, r.error.c_str());
        return b;
    }
    const DevCfg &dc = *r.dc;
    std::snprintf(b, sizeof b,
                  "%s dc=%016llx records=%016llx/%zu tab=%016llx/%zu cols=%016llx tab2=%016llx/%zu cols2=%016llx col_len=%016llx hyb=%016llx/%zu "
                  "rh=%.17g,%.17g,%.17g ed_reuse_fit=%d terms2=%d harm_feed=%d rec_in_lds=%d dcm_incr=%d coop_frac=%.17g swap=%d:%d,%d,%d,%d:%g,%g,%g,%g",
                  tag.c_str(), (unsigned long long)fnv1a(&dc, sizeof dc), (unsigned long long)digest(r.records), r.records.size(),
                  (unsigned long long)digest(r.tab), r.tab.size(), (unsigned long long)digest(r.cols), (unsigned long long)digest(r.tab2), r.tab2.size(),
                  (unsigned long long)digest(r.cols2), (unsigned long long)digest(r.col_len), (unsigned long long)digest(r.hyb), r.hyb.size(), r.rh[0],
                  r.rh[1], r.rh[2], r.ed_reuse_fit, r.terms2, dc.harm_feed, dc.rec_in_lds, dc.dcm_incr, dc.coop_frac, r.swap_n_chain, r.swap_seg[0],
                  r.swap_seg[1], r.swap_seg[2], r.swap_seg[3], r.swap_sign[0], r.swap_sign[1], r.swap_sign[2], r.swap_sign[3]);
    return b;
}

// nyx_hip_ctx_create on a 256-CU device, up to the uploads
inline Result build(const Case &c, LdsBytesFn lds) {
    Result r;
    CtxBuild b;
    if ((r.rc = build_context(c.cfg->cfg, c.tune, lds, b)) != NYX_HIP_RC_OK) { r.error = b.error; return r; }
    std::memcpy(r.dc.get(), &b.dc, sizeof(DevCfg));
    r.records = b.records; r.tab = b.tab; r.cols = b.cols; r.tab2 = b.tab2; r.cols2 = b.cols2; r.col_len = b.col_len;
    std::memcpy(r.rh, b.role_handicap, sizeof r.rh);
    r.ed_reuse_fit = b.ed_reuse_fit; r.terms2 = b.terms2; r.swap_n_chain = b.swap_n_chain;
    std::memcpy(r.swap_seg, b.swap_seg, sizeof r.swap_seg);
    std::memcpy(r.swap_sign, b.swap_sign, sizeof r.swap_sign);
    const WeightMap none;
    SchedShape shape;
    plan_first_schedule(PlanInputs{c.tune, r.col_len, r.rh, r.terms2, r.ed_reuse_fit, 256, 0, -1, none}, *r.dc, shape, b.harm_feed);
    if (!r.tab.empty()) {
        int64_t vec_off = 0;
        build_hybrid(r.tab, r.hyb, vec_off);
    }
    return r;
}

inline std::vector<Case> cases() {
    std::vector<Case> v;
    for (lpc::Shape &s : lpc::shapes()) v.push_back(Case{s.name, std::move(s.cfg), NYX_HIP_TUNING_DEFAULT});
    // configs[1]'s force model on an 8x8 field, changed by `f`
    auto add = [&](const char *name, void (*f)(Config &, nyx_hip_tuning_t &), int degree = 8, uint32_t flags = 0) {
        v.push_back(Case{name, lpc::earth_sun_moon(degree, flags), NYX_HIP_TUNING_DEFAULT});
        if (f) f(*v.back().cfg, v.back().tune);
    };
    auto drag = [](Config &c, int density) {
        c.drag = nyx_hip_drag_t{density, 0, 3.614e-13, 700000.0, 700000.0, 1e6, 6378.1363, lpc::iau_rotation()};
        c.cfg.drag = &c.drag;
    };
    auto tides = [](Config &c, const nyx_hip_rotation_t &rot) {
        c.tides.k2 = 0.3019; c.tides.k3 = 0.093; c.tides.mu_km3_s2 = 398600.4415; c.tides.eq_radius_km = 6378.1363; c.tides.rotation = rot;
        c.tides.n_perturbers = 2;
        c.tides.perturber_body[0] = lpc::MOON; c.tides.compute_degree_3[0] = 1;
        c.tides.perturber_body[1] = lpc::SUN;
        c.cfg.tides = &c.tides;
    };
    // ---- branches of a successful build
    add("iau_no_nutation", nullptr);
    add("iau_no_nutation+dbg0x4000", [](Config &, nyx_hip_tuning_t &t) { t.debug_flags = 0x4000; });
    add("iau_nutation", [](Config &c, nyx_hip_tuning_t &) { c.field[0].rotation = lpc::iau_rotation(3); });
    add("euler_cheby", [](Config &c, nyx_hip_tuning_t &) { c.field[0].rotation.kind = NYX_HIP_ROT_EULER_CHEBY; c.field[0].rotation.euler_segment = 2; c.field[0].rotation.base_dcm[4] = 1.0; });
    add("dbg0x8000+0x2000000", [](Config &, nyx_hip_tuning_t &t) { t.debug_flags = 0x8000 | 0x2000000; });
    add("stm", nullptr, 8, NYX_HIP_FLAG_STM);
    add("stm_textbook", nullptr, 8, NYX_HIP_FLAG_STM | NYX_HIP_FLAG_STM_TEXTBOOK);
    add("stm_state_ctrl", [](Config &c, nyx_hip_tuning_t &) { c.cfg.opts.error_ctrl = NYX_HIP_RSS_CARTESIAN_STATE; }, 8, NYX_HIP_FLAG_STM);
    add("drag_const", nullptr);
    v.back().cfg->cfg.gravity = nullptr;
    drag(*v.back().cfg, 0);
    add("drag_exp+field", nullptr);
    drag(*v.back().cfg, 1);
    add("drag_stdatm+field", nullptr);
    drag(*v.back().cfg, 2);
    add("tides_deg3+field", nullptr);
    tides(*v.back().cfg, lpc::iau_rotation());
    add("tides_only_nutation", nullptr);
    v.back().cfg->cfg.gravity = nullptr;
    tides(*v.back().cfg, lpc::iau_rotation(2));
    add("tides+drag", nullptr);
    v.back().cfg->cfg.gravity = nullptr;
    drag(*v.back().cfg, 1);
    tides(*v.back().cfg, lpc::iau_rotation());
    add("grav_offset_moon", [](Config &c, nyx_hip_tuning_t &) { c.field[0].offset_body = lpc::MOON + 1; });
    add("grav_offset_centre", [](Config &c, nyx_hip_tuning_t &) { c.field[0].offset_body = lpc::EARTH + 1; });
    add("grav2_offset_jupiter", [](Config &c, nyx_hip_tuning_t &) { lpc::set_field(c, 1, 6, lpc::JUPITER + 1); });
    add("grav2_centre", [](Config &c, nyx_hip_tuning_t &) { lpc::set_field(c, 1, 5); c.field[1].order = 3; });
    add("state_frame_moon", [](Config &c, nyx_hip_tuning_t &) { c.cfg.state_frame_body = lpc::MOON; });
    add("state_frame_jupiter", [](Config &c, nyx_hip_tuning_t &) { c.cfg.state_frame_body = lpc::JUPITER; });
    add("segment_26_coefficients", [](Config &c, nyx_hip_tuning_t &) { lpc::add_segment(c, 26, 3); });
    add("segment_16_coefficients", [](Config &c, nyx_hip_tuning_t &) { lpc::add_segment(c, 16, 3); });
    add("records_past_24k", [](Config &c, nyx_hip_tuning_t &) { lpc::add_segment(c, 13, 80); });
    add("records_past_8m_padded", [](Config &c, nyx_hip_tuning_t &) { lpc::add_segment(c, 13, 25000); });
    add("feed0", [](Config &, nyx_hip_tuning_t &t) { t.harmonics_feed = 0; }, 70);
    add("feed1", [](Config &, nyx_hip_tuning_t &t) { t.harmonics_feed = 1; });
    add("feed2", [](Config &, nyx_hip_tuning_t &t) { t.harmonics_feed = 2; });
    add("feed3", [](Config &, nyx_hip_tuning_t &t) { t.harmonics_feed = 3; });
    add("feed_auto_deg100", nullptr, 100);
    add("feed3_no_field", [](Config &c, nyx_hip_tuning_t &t) { c.cfg.gravity = nullptr; t.harmonics_feed = 3; });
    add("role_duties", [](Config &, nyx_hip_tuning_t &t) { t.role_duties[0] = 60.0; t.role_duties[1] = 600.0; t.role_duties[2] = 52.0; }, 70);
    add("coop_fraction0.01", [](Config &, nyx_hip_tuning_t &t) { t.coop_fraction = 0.01; }, 70);
    add("coop_fraction0.95", [](Config &, nyx_hip_tuning_t &t) { t.coop_fraction = 0.95; }, 70);
    add("coop_fraction0.4", [](Config &, nyx_hip_tuning_t &t) { t.coop_fraction = 0.4; }, 70);
    add("epoch_data_reuse0", [](Config &, nyx_hip_tuning_t &t) { t.epoch_data_reuse = 0; });
    add("dp45_odd_stages", [](Config &c, nyx_hip_tuning_t &) { c.cfg.opts.method = NYX_HIP_DP45; });
    add("rk4_fixed", [](Config &c, nyx_hip_tuning_t &) { c.cfg.opts.method = NYX_HIP_RK4; c.cfg.opts.fixed_step = 1; c.cfg.opts.min_step_ns = 1234567891; });
    add("srp_estimate_shadow_moon", [](Config &c, nyx_hip_tuning_t &) { c.srp.estimate = 1; c.srp.shadow_body[c.srp.n_shadow_bodies++] = lpc::MOON; });
    // ---- refusals, in the order the builder checks them
    add("err_method", [](Config &c, nyx_hip_tuning_t &) { c.cfg.opts.method = 6; });
    add("err_stm_error_ctrl", [](Config &c, nyx_hip_tuning_t &) { c.cfg.opts.error_ctrl = NYX_HIP_RSS_STATE; }, 8, NYX_HIP_FLAG_STM);
    add("err_textbook_without_stm", nullptr, 8, NYX_HIP_FLAG_STM_TEXTBOOK);
    add("err_drag_stm", nullptr, 8, NYX_HIP_FLAG_STM);
    drag(*v.back().cfg, 0);
    add("err_drag_frame", nullptr);
    drag(*v.back().cfg, 0);
    v.back().cfg->drag.rotation.w_deg[0] = 1.0;
    add("err_tides_frame", nullptr);
    tides(*v.back().cfg, lpc::iau_rotation(1));
    add("err_tides_model", nullptr);
    tides(*v.back().cfg, lpc::iau_rotation());
    v.back().cfg->tides.mu_km3_s2 = 0.0;
    add("err_counts", [](Config &c, nyx_hip_tuning_t &) { c.cfg.n_point_masses = NYX_HIP_MAX_BODIES + 1; });
    add("err_n_chain", [](Config &c, nyx_hip_tuning_t &) { c.bodies[lpc::SUN].n_chain = 5; });
    add("err_segment_interval", [](Config &c, nyx_hip_tuning_t &) { c.segments[1].interval_s = 0.0; });
    add("err_segment_33_coefficients", [](Config &c, nyx_hip_tuning_t &) { lpc::add_segment(c, 33); });
    add("err_rotation_kind", [](Config &c, nyx_hip_tuning_t &) { c.field[0].rotation.kind = 7; });
    add("err_rotation_nutation", [](Config &c, nyx_hip_tuning_t &) { c.field[0].rotation.n_nut_prec = NYX_HIP_MAX_NUT_PREC + 1; });
    add("err_rotation_euler_segment", [](Config &c, nyx_hip_tuning_t &) { c.field[0].rotation.kind = NYX_HIP_ROT_EULER_CHEBY; c.field[0].rotation.euler_segment = 5; });
    add("err_debug_flags_retired", [](Config &, nyx_hip_tuning_t &t) { t.debug_flags = 0x800 | 0x40000 | 0x1000; });
    add("err_state_frame_body", [](Config &c, nyx_hip_tuning_t &) { c.cfg.state_frame_body = 6; });
    add("err_state_frame_chain", [](Config &c, nyx_hip_tuning_t &) { c.cfg.state_frame_body = lpc::JUPITER; c.bodies[lpc::JUPITER].chain_segment[1] = 5; });
    add("err_point_mass_body", [](Config &c, nyx_hip_tuning_t &) { c.cfg.point_mass_body[1] = 9; });
    add("err_point_mass_slots", [](Config &c, nyx_hip_tuning_t &) {
        lpc::add_body(c, 1.0, 1.0, {0}, {+1});
        lpc::add_body(c, 2.0, 1.0, {1}, {+1});
        lpc::point_masses(c, {lpc::JUPITER, 4, 5});
    });
    add("err_srp_sun_central", [](Config &c, nyx_hip_tuning_t &) { c.srp.sun_body = lpc::EARTH; });
    add("err_shadow_count", [](Config &c, nyx_hip_tuning_t &) { c.srp.n_shadow_bodies = DEV_MAX_SLOTS + 1; });
    add("err_shadow_body", [](Config &c, nyx_hip_tuning_t &) { c.srp.shadow_body[0] = -1; });
    add("err_tidal_perturber_central", nullptr);
    tides(*v.back().cfg, lpc::iau_rotation());
    v.back().cfg->tides.perturber_body[1] = lpc::EARTH;
    add("err_too_many_segments", [](Config &c, nyx_hip_tuning_t &) { for (int k = 0; k < 4; ++k) lpc::add_segment(c, 9); });
    add("err_chain_segment", [](Config &c, nyx_hip_tuning_t &) { c.bodies[lpc::MOON].chain_segment[1] = 5; });
    add("err_gravity_degree", [](Config &c, nyx_hip_tuning_t &) { c.field[0].degree = 0; });
    add("err_offset_body", [](Config &c, nyx_hip_tuning_t &) { c.field[0].offset_body = 7; });
    add("err_offset_body_slots", [](Config &c, nyx_hip_tuning_t &) {
        lpc::add_body(c, 1.0, 1.0, {0}, {+1});
        lpc::point_masses(c, {lpc::JUPITER, 4});
        lpc::add_body(c, 2.0, 1.0, {1}, {+1});
        c.field[0].offset_body = 6;
    });
    add("err_offset_chain", [](Config &c, nyx_hip_tuning_t &) { c.field[0].offset_body = lpc::JUPITER + 1; c.bodies[lpc::JUPITER].chain_segment[2] = -1; });
    add("err_gravity2_alone", [](Config &c, nyx_hip_tuning_t &) { lpc::set_field(c, 1, 4); c.cfg.gravity = nullptr; });
    add("err_gravity2_degree", [](Config &c, nyx_hip_tuning_t &) { lpc::set_field(c, 1, 4); c.field[1].degree = 0; });
    add("err_offset2_body", [](Config &c, nyx_hip_tuning_t &) { lpc::set_field(c, 1, 4, 8); });
    add("err_offset2_chain", [](Config &c, nyx_hip_tuning_t &) { lpc::set_field(c, 1, 4, lpc::JUPITER + 1); c.bodies[lpc::JUPITER].chain_segment[0] = 8; });
    add("err_drag_density", nullptr);
    drag(*v.back().cfg, 3);
    return v;
}

}  // namespace cbc

int main(int argc, char **argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: ctx_build_check OUT\n"); return 2; }
    FILE *out = std::fopen(argv[1], "w");
    if (!out) return 2;
    int n = 0;
    for (const cbc::Case &c : cbc::cases())
        for (const cbc::Fake &f : cbc::kFakes) {
            std::fprintf(out, "%s\n", cbc::result_line(c.name + " " + f.name, cbc::build(c, f.fn)).c_str());
            ++n;
        }
    std::fclose(out);
    std::printf("%d builds\nok\n", n);
    return 0;
}
