// Stand-alone check of the host side of the helpers' resident feed (nyx_amd/csrc/launch_plan.h: run_stream_groups, helper_stage_fits,
// select_helper_feed; nyx_amd/csrc/ctx_build.h: build_run_stream) - g++ only, no HIP, no GPU (tests/test_helper_resident_host.py).
// For configs[1]'s force model on fields of degree 24 .. 150 and the BASELINE ensemble sizes, planned as a launch plans them:
//   1. the block a helper stages is the vector side of the helpers' run stream, group for group: run_stream_groups() is the size
//      build_run_stream() arrives at, every range of every helper wave starts a group of its own, and row q of column c lies at lane
//      q % 16 of its group's four 128-byte lines with the t3..t6 of the entry table - the rows of the schedule's columns, nothing else;
//   2. the selection follows the fit rule: resident exactly for a cooperative launch in the claim mode with a one-part hand-off of
//      sixteen-wave workgroups whose block is at most DEV_HELPER_STAGE_MAX bytes, and never with tuning.helper_resident = 0;
//   3. the carve and the largest block fit the LDS of a workgroup, and the headline shape is selected while config 5's is not.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../nyx_amd/csrc/ctx_build.h"
#include "launch_plan_cases.h"

static int g_fail = 0;
#define CHECK(cond, ...)                                                              \
    do {                                                                              \
        if (!(cond)) {                                                                \
            if (++g_fail <= 20) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                             \
    } while (0)

struct Ctx {  // what nyx_hip_ctx keeps for the planner, and the tables the run streams are built from
    nyx_hip_tuning_t tune;
    std::unique_ptr<DevCfg> dc{new DevCfg};
    std::vector<int32_t> col_len;
    std::vector<HarmEntry> tab;
    std::vector<ColHdr> cols;
    double rh[3] = {0.0, 0.0, 0.0};
    int terms2 = 0, ed_reuse_fit = 0, n_cu = 0;
    WeightMap weights;
    SchedShape shape;
    PlanInputs in() const { return PlanInputs{tune, col_len, rh, terms2, ed_reuse_fit, n_cu, 0, -1, weights}; }
};

static void create(Ctx &c, const lpc::Config &cfg, const nyx_hip_tuning_t &tune, int n_cu) {
    c.tune = tune;
    CtxBuild b;
    if (build_context(cfg.cfg, tune, lpc::lds_room, b) != NYX_HIP_RC_OK) { std::printf("FAIL: %s\n", b.error.c_str()); std::exit(1); }
    std::memcpy(c.dc.get(), &b.dc, sizeof(DevCfg));
    c.col_len = b.col_len; c.tab = b.tab; c.cols = b.cols;
    c.terms2 = b.terms2;
    std::memcpy(c.rh, b.role_handicap, sizeof c.rh);
    c.ed_reuse_fit = b.ed_reuse_fit;
    c.n_cu = n_cu;
    c.shape = SchedShape();
    c.weights.clear();
    plan_first_schedule(c.in(), *c.dc, c.shape, b.harm_feed);
}

// 1. the staged block of the helper schedules in `c`, against the tables
static int64_t check_layout(const Ctx &c, const char *tag) {
    const DevCfg &dc = *c.dc;
    std::vector<double> hyb;
    std::vector<ColHdr> cols_x;
    int64_t vec_off = 0;
    build_run_stream(c.cols, c.tab, dc.sched, {DEV_SCHED_HELPER, DEV_SCHED_HELPER2}, hyb, vec_off, cols_x);
    const int64_t groups = run_stream_groups(dc.sched, {DEV_SCHED_HELPER, DEV_SCHED_HELPER2}, c.col_len);
    CHECK(groups * HYB_GROUP == (int64_t)hyb.size() - vec_off, "%s: %lld groups, stream holds %lld doubles", tag, (long long)groups, (long long)(hyb.size() - vec_off));
    CHECK(helper_stage_bytes(groups) == groups * 512, "%s", tag);
    const double *vec = hyb.data() + vec_off;
    int64_t rows = 0, want_rows = 0;
    for (int k : {DEV_SCHED_HELPER, DEV_SCHED_HELPER2})
        for (int w = 0; w < DEV_MAX_WAVES; ++w)
            for (int r = 0; r < dc.sched[k].n_ranges[w]; ++r) {
                const int c0 = dc.sched[k].range_c0[w][r];
                CHECK(cols_x[c0].start % 16 == 0, "%s: range of wave %d starts inside a group", tag, w);
                int64_t at = cols_x[c0].start;
                for (int col = c0; col < c0 + dc.sched[k].range_cnt[w][r]; ++col) {
                    CHECK(cols_x[col].start == at && cols_x[col].rows == c.col_len[col], "%s: column %d", tag, col);
                    for (int q = 0; q < c.col_len[col]; ++q, ++at, ++rows) {
                        const HarmEntry &e = c.tab[(size_t)c.cols[col].start + q];
                        const double *g = vec + (at / 16) * HYB_GROUP + at % 16;
                        CHECK(at / 16 < groups - 2, "%s: row past the block's last full group", tag);
                        CHECK(g[0] == e.t3 && g[16] == e.t4 && g[32] == e.t5 && g[48] == e.t6, "%s: column %d row %d", tag, col, q);
                    }
                    want_rows += c.col_len[col];
                }
            }
    CHECK(rows == want_rows && rows > 0, "%s: %lld rows staged, %lld in the columns", tag, (long long)rows, (long long)want_rows);
    // nothing but those rows and zero padding: the doubles of the block that are not zero are at most four per row
    int64_t nonzero = 0;
    for (int64_t q = 0; q < groups * HYB_GROUP; ++q) nonzero += vec[q] != 0.0;
    CHECK(nonzero <= 4 * rows, "%s: %lld non-zero doubles for %lld rows", tag, (long long)nonzero, (long long)rows);
    return groups;
}

int main() {
    static_assert(DEV_HELPER_LDS_BYTES % 128 == 0, "the block behind the carve is read as 128-byte lines");
    CHECK((size_t)DEV_HELPER_LDS_BYTES + DEV_HELPER_STAGE_MAX <= kKernelLdsMax, "carve + largest block exceed a workgroup's LDS");
    Ctx c;
    long cases = 0, resident = 0;
    for (int deg : {24, 33, 40, 56, 70, 97, 150}) {
        const std::unique_ptr<lpc::Config> cfg = lpc::earth_sun_moon(deg);
        for (int variant = 0; variant < 4; ++variant) {
            nyx_hip_tuning_t tune = NYX_HIP_TUNING_DEFAULT;
            if (variant == 1) tune.helper_resident = 0;
            if (variant == 2) tune.debug_flags = 0x8000000;  // no fan-out mode: small ensembles in the claim mode
            if (variant == 3) tune.debug_flags = 0x80000;    // one-part hand-off (and no fan-out mode) whatever the field
            for (int64_t n : {64, 520, 700, 1250, 2500, 5000, 6250, 10000, 16384}) {
                create(c, *cfg, tune, 256);
                const LaunchPlan p = plan_launch(c.in(), *c.dc, c.shape, n, false);
                const std::string tag = "deg" + std::to_string(deg) + " v" + std::to_string(variant) + " n=" + std::to_string(n);
                ++cases;
                const bool claim16 = p.coop.run && !p.coop.fan && p.coop.parts == 1 && p.n_waves == DEV_MAX_WAVES;
                if (!p.coop.run || p.coop.fan) { CHECK(p.staged_groups == 0 && c.dc->hres_groups == 0, "%s: resident without claim-mode helpers", tag.c_str()); continue; }
                const int64_t groups = check_layout(c, tag.c_str());
                const bool want = claim16 && tune.helper_resident != 0 && helper_stage_bytes(groups) <= DEV_HELPER_STAGE_MAX;
                CHECK((p.staged_groups > 0) == want, "%s: staged %d, block %lld bytes", tag.c_str(), p.staged_groups, (long long)helper_stage_bytes(groups));
                if (claim16) CHECK(c.dc->hres_groups == p.staged_groups, "%s: the descriptor's word is not the launch's", tag.c_str());
                if (want) { CHECK(p.staged_groups == groups, "%s", tag.c_str()); ++resident; }
                // a second plan of the same launch changes nothing (the selection is a function of the plan)
                const LaunchPlan p2 = plan_launch(c.in(), *c.dc, c.shape, n, false);
                CHECK(!p2.rebuilt && (p2.staged_groups > 0) == want, "%s: second plan", tag.c_str());
            }
        }
    }
    std::printf("%ld planned cases, %ld with the resident feed\n", cases, resident);
    {   // the headline shape takes it; a launch that works alone drops it again; config 5's block does not fit
        const std::unique_ptr<lpc::Config> cfg = lpc::earth_sun_moon(70);
        create(c, *cfg, NYX_HIP_TUNING_DEFAULT, 256);
        LaunchPlan p = plan_launch(c.in(), *c.dc, c.shape, 10000, false);
        const int64_t bytes = helper_stage_bytes(c.dc->hres_groups);
        CHECK(p.coop.run && p.coop.helpers == 99 && c.dc->hres_groups > 0 && p.rebuilt, "headline: %d groups", c.dc->hres_groups);
        std::printf("headline (70x70, 10 000 trajectories): %d groups = %lld bytes behind a carve of %d\n", c.dc->hres_groups, (long long)bytes, (int)DEV_HELPER_LDS_BYTES);
        // a launch that works alone stages nothing and leaves the descriptor as it is: alternating launches rebuild and upload nothing
        const int32_t kept = c.dc->hres_groups;
        p = plan_launch(c.in(), *c.dc, c.shape, 16384, false);
        CHECK(!p.coop.run && p.staged_groups == 0 && c.dc->hres_groups == kept && !p.rebuilt, "full chip: staged %d rebuilt %d", p.staged_groups, (int)p.rebuilt);
        p = plan_launch(c.in(), *c.dc, c.shape, 10000, false);
        CHECK(p.coop.run && p.staged_groups == kept && !p.rebuilt, "headline again: staged %d rebuilt %d", p.staged_groups, (int)p.rebuilt);
        const auto shapes = lpc::shapes();
        create(c, *shapes[3].cfg, NYX_HIP_TUNING_DEFAULT, 256);  // config 5: 150x150
        p = plan_launch(c.in(), *c.dc, c.shape, 6250, false);
        CHECK(p.coop.run && p.staged_groups == 0, "config 5: %d groups", p.staged_groups);
        nyx_hip_tuning_t one = NYX_HIP_TUNING_DEFAULT;
        one.debug_flags = 0x80000;
        create(c, *shapes[3].cfg, one, 256);
        p = plan_launch(c.in(), *c.dc, c.shape, 6250, false);
        const int64_t g5 = run_stream_groups(c.dc->sched, {DEV_SCHED_HELPER, DEV_SCHED_HELPER2}, c.col_len);
        CHECK(p.coop.run && p.coop.parts == 1 && helper_stage_bytes(g5) > DEV_HELPER_STAGE_MAX && p.staged_groups == 0 && c.dc->hres_groups == 0, "config 5, one part: %lld bytes", (long long)helper_stage_bytes(g5));
        std::printf("config 5 (150x150, 6 250 trajectories, one part): %lld bytes, not staged\n", (long long)helper_stage_bytes(g5));
    }
    if (g_fail) { std::printf("%d failures\n", g_fail); return 1; }
    std::printf("ok\n");
    return 0;
}
