// Stand-alone check of the launch planner (nyx_amd/csrc/launch_plan.h) - g++ only, no HIP, no GPU (tests/test_launch_plan.py).
//   launch_plan_check PLANS_OUT
// writes the plan of every case at 256 CUs to PLANS_OUT, one line each (compared with tests/golden/launch_plans.txt.gz by the test),
// checks the invariants below on every case at 256, 304 and 80 CUs, and prints "ok" last when they all hold.
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

struct Ctx {  // what nyx_hip_ctx keeps for the planner
    nyx_hip_tuning_t tune;
    std::unique_ptr<DevCfg> dc{new DevCfg};
    std::vector<int32_t> col_len;
    double rh[3] = {0.0, 0.0, 0.0};
    int terms2 = 0, ed_reuse_fit = 0, n_cu = 0;
    WeightMap weights;
    SchedShape shape;
    PlanInputs in() const { return PlanInputs{tune, col_len, rh, terms2, ed_reuse_fit, n_cu, 0, -1, weights}; }
};

// nyx_hip_ctx_create, as far as the planner is concerned
static void create(Ctx &c, const lpc::Shape &sh, const nyx_hip_tuning_t &tune, bool inject, int n_cu) {
    c.tune = tune;
    CtxBuild b;
    if (build_context(sh.cfg->cfg, tune, lpc::lds_room, b) != NYX_HIP_RC_OK) {
        std::printf("FAIL %s: %s\n", sh.name.c_str(), b.error.c_str());
        std::exit(1);
    }
    std::memcpy(c.dc.get(), &b.dc, sizeof(DevCfg));
    c.col_len = b.col_len;
    c.terms2 = b.terms2;
    std::memcpy(c.rh, b.role_handicap, sizeof c.rh);
    c.ed_reuse_fit = b.ed_reuse_fit;
    c.n_cu = n_cu;
    c.shape = SchedShape();
    c.weights.clear();
    plan_first_schedule(c.in(), *c.dc, c.shape, b.harm_feed);
    if (inject) lpc::inject_weights(c.weights);
}

// every column 1..n_cols exactly once over the given schedules, waves < n_waves only
static bool dealt_once(const DevCfg &dc, std::initializer_list<int> ids, int first_fan = -1, int n_fan = 0) {
    std::vector<int> seen(dc.n_cols + 2, 0);
    std::vector<int> all(ids);
    for (int p = 0; p < n_fan; ++p) all.push_back(first_fan + p);
    for (int k : all)
        for (int w = 0; w < DEV_MAX_WAVES; ++w)
            for (int r = 0; r < dc.sched[k].n_ranges[w]; ++r)
                for (int col = dc.sched[k].range_c0[w][r]; col < dc.sched[k].range_c0[w][r] + dc.sched[k].range_cnt[w][r]; ++col) {
                    if (col < 1 || col > dc.n_cols || w >= dc.n_waves) return false;
                    ++seen[col];
                }
    for (int col = 1; col <= dc.n_cols; ++col)
        if (seen[col] != 1) return false;
    return true;
}

static void invariants(const Ctx &c, const LaunchPlan &p, int64_t n, const std::string &tag) {
    const DevCfg &dc = *c.dc;
    const CoopPlan &cp = p.coop;
    const char *t = tag.c_str();
    CHECK(dc.n_waves == p.n_waves, "%s", t);
    for (int k = 0; k < DEV_N_SCHED; ++k)
        for (int w = 0; w < DEV_MAX_WAVES; ++w) CHECK(dc.sched[k].n_ranges[w] >= 0 && dc.sched[k].n_ranges[w] <= DEV_MAX_RANGES, "%s s%d w%d", t, k, w);
    if (dc.has_grav) CHECK(dealt_once(dc, {DEV_SCHED_SOLO}), "%s: SOLO", t);
    if (dc.pipe)  // the pipelined integrator wave walks nothing
        for (int k : {DEV_SCHED_SOLO, DEV_SCHED_PRIMARY}) CHECK(dc.sched[k].n_ranges[0] == 0, "%s: integrator walks s%d", t, k);
    const int64_t n_own = (n + DEV_LANES - 1) / DEV_LANES;
    CHECK(!cp.run || (cp.n_own == n_own && cp.base == n_own && cp.helpers > 0 && dc.coop_ok && cp.coop_frac == dc.coop_frac), "%s", t);
    CHECK(!cp.run || cp.base + cp.helpers <= c.n_cu, "%s: more workgroups than CUs", t);
    if (cp.run && cp.fan) {
        CHECK(dealt_once(dc, {DEV_SCHED_PRIMARY}, DEV_SCHED_FAN0, cp.parts), "%s: PRIMARY + FAN", t);
        CHECK(cp.parts == std::min<int64_t>(DEV_FAN_MAX, (c.n_cu - n_own) / n_own) && cp.helpers == n_own * cp.parts, "%s: fan helpers", t);
        CHECK(cp.answers == n_own * cp.parts, "%s", t);
    } else if (cp.run) {
        CHECK(dealt_once(dc, {DEV_SCHED_PRIMARY, DEV_SCHED_HELPER, DEV_SCHED_HELPER2}), "%s: PRIMARY + HELPER", t);
        CHECK(cp.answers == (cp.parts == 2 ? n_own : 0), "%s", t);
    }
    // the mailbox block launch() acquires holds max(boxes, answers, 256) of each
    CHECK(!cp.run || (cp.boxes == n_own && std::max<int64_t>({cp.boxes, cp.answers, 256}) >= n_own * (cp.fan ? cp.parts : 1)), "%s: mailboxes", t);
}

static std::string line(const Ctx &c, const LaunchPlan &p, const std::string &tag) {
    const CoopPlan &cp = p.coop;
    return lpc::plan_line(tag, *c.dc, p.n_waves, p.quad, cp.run, cp.helpers, cp.base, cp.parts, cp.fan);
}

int main(int argc, char **argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: launch_plan_check PLANS_OUT\n"); return 2; }
    FILE *out = std::fopen(argv[1], "w");
    if (!out) return 2;
    const auto shapes = lpc::shapes();
    const auto vars = lpc::variants();
    Ctx c;
    long cases = 0;
    // 1 + 2. every shape x tuning x size from a fresh context, and one context over a sequence of sizes
    for (int n_cu : {256, 304, 80})
        for (const auto &sh : shapes)
            for (const auto &v : vars) {
                for (int64_t n : lpc::kSizes) {
                    create(c, sh, v.tune, v.inject_weights, n_cu);
                    const LaunchPlan p = plan_launch(c.in(), *c.dc, c.shape, n, false);
                    const std::string tag = sh.name + " " + v.name + " n=" + std::to_string(n);
                    invariants(c, p, n, tag + " cu=" + std::to_string(n_cu));
                    if (n_cu == 256) std::fprintf(out, "%s\n", line(c, p, tag).c_str());
                    ++cases;
                }
                create(c, sh, v.tune, v.inject_weights, n_cu);
                int step = 0;
                for (int64_t n : lpc::kSequence) {
                    const LaunchPlan p = plan_launch(c.in(), *c.dc, c.shape, n, false);
                    const std::string tag = sh.name + " " + v.name + " seq" + std::to_string(step++) + " n=" + std::to_string(n);
                    invariants(c, p, n, tag + " cu=" + std::to_string(n_cu));
                    if (n_cu == 256) std::fprintf(out, "%s\n", line(c, p, tag).c_str());
                    ++cases;
                }
            }
    std::fclose(out);
    std::printf("%ld planned cases\n", cases);

    // 3. the helper counts tests/test_gpu_fan.py, test_gpu_parity.py and test_gpu_reproducible.py expect of a 256-CU device
    {
        const lpc::Shape &sh = shapes[0];  // configs[1], 70x70
        auto helpers = [&](int64_t n, int n_cu) {
            create(c, sh, NYX_HIP_TUNING_DEFAULT, false, n_cu);
            return plan_launch(c.in(), *c.dc, c.shape, n, false).coop.helpers;
        };
        CHECK(helpers(64, 256) == 8 && helpers(1250, 256) == 160 && helpers(2500, 256) == 200 && helpers(5000, 256) == 158, "fan-out helper counts");
        CHECK(helpers(640, 256) == 80 && helpers(128, 256) == 16 && helpers(10000, 256) == 99, "helper counts");
        create(c, sh, NYX_HIP_TUNING_DEFAULT, false, 256);
        int64_t h[3];
        int k = 0;
        for (int64_t n : {1280, 10000, 1280}) h[k++] = plan_launch(c.in(), *c.dc, c.shape, n, false).coop.helpers;
        CHECK(h[0] == 160 && h[1] == 99 && h[2] == 160, "one context, 1280 / 10000 / 1280: %lld %lld %lld", (long long)h[0], (long long)h[1], (long long)h[2]);
        // 304 CUs, 33 owners, 8 parts = 264 answer blocks, more than the 256 of the smallest mailbox block
        create(c, sh, NYX_HIP_TUNING_DEFAULT, false, 304);
        const CoopPlan cp = plan_launch(c.in(), *c.dc, c.shape, 33 * 64, false).coop;
        CHECK(cp.run && cp.fan && cp.n_own == 33 && cp.parts == 8 && cp.answers == 264 && std::max<int64_t>({cp.boxes, cp.answers, 256}) == 264,
              "304 CUs: %lld answers", (long long)cp.answers);
        std::printf("helper counts at 256 CUs: 8 / 160 / 200 / 158, 80, 16, 99; 304 CUs x 33 owners: %lld answer blocks\n", (long long)cp.answers);
    }

    // 4. no claim-mode or fan-out build fails at default tuning: degrees 8 .. 150 (configs[1]'s force model), every fan-out width, both
    //    claim-mode part counts at every helper share plan_cooperation can derive, and a fresh plan at every BASELINE size on 256 CUs
    {
        long builds = 0;
        for (int deg = 8; deg <= 150; ++deg) {
            const lpc::Shape sh{"deg" + std::to_string(deg), lpc::earth_sun_moon(deg)};  // (configs[1]'s force model)
            for (int64_t n : lpc::kSizes) {
                create(c, sh, NYX_HIP_TUNING_DEFAULT, false, 256);
                const LaunchPlan p = plan_launch(c.in(), *c.dc, c.shape, n, false);
                invariants(c, p, n, sh.name + " n=" + std::to_string(n));
                const int64_t n_own = (n + 63) / 64, free_cus = 256 - n_own;
                const bool gate = p.n_waves == DEV_MAX_WAVES && n_own + 8 <= 256;
                // a fan-out plan where the CU count asks for one (no fall-back to the claim mode), helpers wherever the gate lets them
                if (gate && c.dc->n_cols <= 96 && free_cus >= 2 * n_own) CHECK(p.coop.fan && p.coop.run, "%s n=%lld: fan-out build failed", sh.name.c_str(), (long long)n);
                if (gate) CHECK(c.dc->coop_ok, "%s n=%lld: build failed", sh.name.c_str(), (long long)n);
                ++builds;
            }
            create(c, sh, NYX_HIP_TUNING_DEFAULT, false, 256);
            if (pick_waves(c.in(), *c.dc, 10000) != DEV_MAX_WAVES) continue;  // (below degree 24: eight-wave workgroups, never cooperative)
            for (int K = 2; K <= DEV_FAN_MAX; ++K) {
                SchedShape s; s.coop_fan = true; s.coop_parts = K;
                build_schedule(c.in(), *c.dc, s, DEV_MAX_WAVES);
                CHECK(c.dc->coop_ok && dealt_once(*c.dc, {DEV_SCHED_PRIMARY}, DEV_SCHED_FAN0, K), "deg %d: fan-out build K=%d failed", deg, K);
                ++builds;
            }
            for (int parts = 1; parts <= 2; ++parts)
                for (int x100 = 10; x100 <= 68; ++x100) {
                    SchedShape s; s.coop_parts = parts;
                    c.dc->coop_frac = x100 / 100.0;
                    build_schedule(c.in(), *c.dc, s, DEV_MAX_WAVES);
                    CHECK(c.dc->coop_ok && dealt_once(*c.dc, {DEV_SCHED_PRIMARY, DEV_SCHED_HELPER, DEV_SCHED_HELPER2}), "deg %d: claim build parts=%d x=%.2f failed", deg, parts, x100 / 100.0);
                    ++builds;
                }
        }
        std::printf("%ld builds of degrees 8..150 at default tuning: none fails\n", builds);
    }
    if (g_fail) { std::printf("%d failures\n", g_fail); return 1; }
    std::printf("ok\n");
    return 0;
}
