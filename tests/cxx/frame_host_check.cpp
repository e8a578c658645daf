// Stand-alone check of the host side of the encounter report (nyx_amd/csrc/series_host.h: check_frame_series, check_frame_context;
// nyx_amd/csrc/frame_args.h: frm_param_needs, frm_needs, frm_reduce_chain) and of the kernel's own per-sample code compiled FOR THE
// HOST (nyx_amd/csrc/frame_dev.h: frm_cheby_pv, frm_shared, frm_bplane, frm_param, frm_value) - g++ only, no HIP, no GPU
// (tests/test_frame_host_cxx.py, which builds it plain and with the address and undefined-behaviour sanitizers).
//   frame_host_check INPUT
// runs the refusals over a table of cases and the chain reduction over hand-made chains, then reads INPUT (text, numbers as
// hexadecimal floats so that every bit arrives):
//   n_seg, then per segment: init_et interval n_rec n_coef and its n_rec * (2 + 3 n_coef) record doubles
//   n_targets, then per target: mu n_chain and n_chain pairs (segment sign)
//   n_cases, then per case: target et_s x y z vx vy vz
// lays the records out twice as the context builder may (layout 0: packed, stride 2 + 3 n_coef; layout 1: sixteen coefficients wide,
// zero-padded, stride 50) and prints per layout and case, walking the kernel's second pass:
//   body LAYOUT CASE x y z vx vy vz status      the chain summed in chain order (%a)
//   slim LAYOUT CASE x y z status               the same without the velocity recurrence: the positions must not move
//   val LAYOUT CASE PARAM value via_frm_value   the translated state's parameter, through the shared intermediates of ALL 25 and alone
// "ok" last.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../nyx_amd/csrc/frame_dev.h"
#include "../../nyx_amd/csrc/series_host.h"

static int g_fail = 0;
#define CHECK(cond, ...)                                                              \
    do {                                                                              \
        if (!(cond)) {                                                                \
            if (++g_fail <= 30) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                             \
    } while (0)

static const int kSeg = 5;   // segments of the pretended context

// the Sun of an Earth-centred almanac: +sun - emb - earth
static nyx_hip_frame_query_t good_query() {
    nyx_hip_frame_query_t q;
    std::memset(&q, 0, sizeof q);
    q.n_params = 3;
    q.param[0] = NYX_HIP_SP_RMAG;
    q.param[1] = NYX_HIP_FRM_B_DOT_T;
    q.param[2] = NYX_HIP_FRM_C3;
    q.step_ns = 1000000000LL;
    q.n_chain = 3;
    q.chain_segment[0] = 2; q.chain_sign[0] = 1;
    q.chain_segment[1] = 1; q.chain_sign[1] = -1;
    q.chain_segment[2] = 0; q.chain_sign[2] = -1;
    q.chain_sign[3] = 1;
    q.mu_km3_s2 = 1.32712440018e11;
    return q;
}

// `why` empty: accepted; else refused with `rc` and a message that holds `why`
static void expect(const char *label, const nyx_hip_ctx *ctx, bool swapped, const nyx_hip_traj_t *t, int64_t n, const nyx_hip_frame_query_t *q,
                   int64_t capacity, const double *values, const int32_t *len, const char *why, int rc = NYX_HIP_RC_BAD_ARG) {
    // (as abi.cpp chains them: the query alone, then what it asks of the context)
    Refusal r = check_frame_series(ctx, t, n, q, capacity, values, len);
    if (!r) r = check_frame_context(*q, kSeg, swapped);
    if (!*why) {
        CHECK(r.rc == NYX_HIP_RC_OK, "%s: refused with '%s'", label, r.msg);
    } else {
        CHECK(r.rc == rc && std::strstr(r.msg, why) != nullptr, "%s: rc %d, message '%s', expected %d '%s'", label, r.rc, r.msg, rc, why);
    }
}

static void refusals() {
    const nyx_hip_ctx *ctx = (const nyx_hip_ctx *)(uintptr_t)1;   // never dereferenced
    int64_t epoch[1] = {0};
    double x[1] = {0};
    int32_t tl[1] = {0};
    nyx_hip_traj_t t;
    std::memset(&t, 0, sizeof t);
    t.capacity = 1;
    t.epoch_ns = epoch;
    t.x_km = t.y_km = t.z_km = t.vx_km_s = t.vy_km_s = t.vz_km_s = x;
    t.len = tl;
    double values[1] = {0.0};
    int32_t len[1] = {0};
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    nyx_hip_frame_query_t q = good_query();
    expect("good", ctx, false, &t, 1, &q, 4, values, len, "");
    expect("n = 0", ctx, false, &t, 0, &q, 4, values, len, "");
    expect("null ctx", nullptr, false, &t, 1, &q, 4, values, len, "null ctx");
    nyx_hip_traj_t bad_t = t;
    bad_t.len = nullptr;
    expect("null array", ctx, false, &bad_t, 1, &q, 4, values, len, "traj: null array");
    expect("null query", ctx, false, &t, 1, nullptr, 4, values, len, "traj_frame_values: null query");
    expect("negative n", ctx, false, &t, -1, &q, 4, values, len, "negative n");
#define CASE(label, mutate, cap, why) do { q = good_query(); mutate; expect(label, ctx, false, &t, 1, &q, cap, values, len, why); } while (0)
    CASE("no parameter", q.n_params = 0, 4, "n_params = 0, 1 .. 8");
    CASE("nine parameters", q.n_params = 9, 4, "n_params = 9, 1 .. 8");
    CASE("unknown parameter", q.param[1] = NYX_HIP_FRM_COUNT, 4, "param[1] = 25 is not a nyx_hip_frame_param");
    CASE("negative parameter", q.param[0] = -1, 4, "param[0] = -1");
    CASE("step 0", q.step_ns = 0, 4, "step_ns must be > 0");
    CASE("capacity 0", (void)0, 0, "capacity must be 1 .. 2^31 - 1");
    CASE("capacity 2^31", (void)0, (int64_t)INT32_MAX + 1, "capacity must be 1 .. 2^31 - 1");
    CASE("the centre itself", q.n_chain = 0, 4, "");
    CASE("chain -1", q.n_chain = -1, 4, "n_chain = -1, 0 .. 4");
    CASE("chain 5", q.n_chain = 5, 4, "n_chain = 5, 0 .. 4");
    CASE("chain 4", (q.n_chain = 4, q.chain_segment[3] = 4), 4, "");
    CASE("segment -1", q.chain_segment[0] = -1, 4, "chain_segment[0] = -1 is not a segment of the context");
    CASE("segment of the context", q.chain_segment[1] = kSeg, 4, "chain_segment[1] = 5 is not a segment of the context (0 .. 4)");
    CASE("sign 0", q.chain_sign[2] = 0, 4, "chain_sign[2] = 0, +1 or -1");
    CASE("sign 2", q.chain_sign[1] = 2, 4, "chain_sign[1] = 2, +1 or -1");
    CASE("a bad link beyond n_chain is not read", (q.chain_segment[3] = 99, q.chain_sign[3] = 7), 4, "");
    CASE("mu 0", q.mu_km3_s2 = 0.0, 4, "mu_km3_s2 must be finite and > 0");
    CASE("mu < 0", q.mu_km3_s2 = -1.0, 4, "mu_km3_s2 must be finite and > 0");
    CASE("mu inf", q.mu_km3_s2 = inf, 4, "mu_km3_s2 must be finite and > 0");
    CASE("mu NaN", q.mu_km3_s2 = nan, 4, "mu_km3_s2 must be finite and > 0");
    // which check wins: the parameters before the step, the step before the chain, the chain before mu, the query before the context
    CASE("parameters before step", (q.n_params = 0, q.step_ns = 0), 4, "n_params");
    CASE("step before chain", (q.step_ns = 0, q.n_chain = 9), 4, "step_ns");
    CASE("chain before mu", (q.chain_sign[0] = 0, q.mu_km3_s2 = 0.0), 4, "chain_sign[0]");
    CASE("the query before the context", (q.chain_segment[0] = kSeg, q.mu_km3_s2 = 0.0), 4, "mu_km3_s2");
    q = good_query();
    expect("null values", ctx, false, &t, 1, &q, 4, nullptr, len, "values and len arrays required");
    expect("null len", ctx, false, &t, 1, &q, 4, values, nullptr, "values and len arrays required");
    q.chain_segment[2] = kSeg;
    expect("outputs before the context", ctx, false, &t, 1, &q, 4, nullptr, len, "values and len arrays required");
    expect("segments before the swap", ctx, true, &t, 1, &q, 4, values, len, "chain_segment[2] = 5");
    q = good_query();
    // the integration-frame swap: the one refusal that is not a bad argument, and the last to fire
    expect("frame swap", ctx, true, &t, 1, &q, 4, values, len, "integration-frame swap", NYX_HIP_RC_UNSUPPORTED);
    q.n_params = 0;
    expect("bad argument before the swap", ctx, true, &t, 1, &q, 4, values, len, "n_params");

    // ---- what each parameter needs
    const int all_rep = REP_NEED_R | REP_NEED_V | REP_NEED_H | REP_NEED_ENERGY | REP_NEED_SMA | REP_NEED_EVEC;
    for (int p : {NYX_HIP_SP_X, NYX_HIP_SP_Y, NYX_HIP_SP_Z}) CHECK(frm_param_needs(p) == 0, "needs of %d", p);
    CHECK(frm_param_needs(NYX_HIP_SP_RMAG) == (REP_NEED_R | FRM_NEED_ELEMENTS), "Rmag needs no velocity");
    for (int p : {NYX_HIP_SP_VX, NYX_HIP_SP_VY, NYX_HIP_SP_VZ}) CHECK(frm_param_needs(p) == FRM_NEED_VELOCITY, "needs of %d", p);
    for (int p = NYX_HIP_SP_VMAG; p < NYX_HIP_FRM_COUNT; ++p) {
        const int k = frm_param_needs(p);
        CHECK(k > 0 && (k & FRM_NEED_VELOCITY) && (k & FRM_NEED_ELEMENTS) && (k & all_rep), "needs of %d = %d", p, k);
        if (p <= NYX_HIP_SP_PERIAPSIS_RADIUS) CHECK((k & all_rep) == report_param_needs(p) && !(k & FRM_NEED_BPLANE), "needs of %d = %d", p, k);
        const bool b = p >= NYX_HIP_FRM_B_DOT_T && p <= NYX_HIP_FRM_B_MAGNITUDE;
        CHECK(((k & FRM_NEED_BPLANE) != 0) == b && (!b || (k & all_rep) == all_rep), "B-plane needs of %d = %d", p, k);
    }
    CHECK(frm_param_needs(NYX_HIP_FRM_C3) == (REP_NEED_R | REP_NEED_V | FRM_NEED_ELEMENTS | FRM_NEED_VELOCITY), "C3");
    CHECK(frm_param_needs(NYX_HIP_FRM_V_INFINITY) & REP_NEED_EVEC, "VInfinity asks the eccentricity whether it exists");
    CHECK(frm_param_needs(NYX_HIP_FRM_COUNT) == -1 && frm_param_needs(-1) == -1, "needs");
    const double unit[6] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0};
    CHECK(std::isnan(frm_value(NYX_HIP_FRM_COUNT, unit, 1.0)) && frm_value(NYX_HIP_SP_ECCENTRICITY, unit, 1.0) == 0.0, "an unknown code is NaN");
}

static void reduction() {
    DevSeg ctx_seg[DEV_MAX_SEG];
    std::memset(ctx_seg, 0, sizeof ctx_seg);
    for (int k = 0; k < DEV_MAX_SEG; ++k) ctx_seg[k].offset = 1000 + k;   // (a tag: which row was copied)
    FrmArgs a;
    std::memset(&a, 0, sizeof a);
    a.q = good_query();
    frm_needs(a);
    CHECK(a.need == (frm_param_needs(NYX_HIP_FRM_B_DOT_T) | REP_NEED_R), "need %d", a.need);
    frm_reduce_chain(a, ctx_seg);
    CHECK(a.n_useg == 3 && a.chain.n_chain == 3, "n_useg = %d", a.n_useg);
    const int want_index[3] = {2, 1, 0};
    for (int u = 0; u < 3; ++u)
        CHECK(a.seg_index[u] == want_index[u] && a.seg[u].offset == 1000 + want_index[u] && a.chain.useg[u] == u, "useg %d = %d", u, a.seg_index[u]);
    CHECK(a.chain.sign[0] == 1.0 && a.chain.sign[1] == -1.0 && a.chain.sign[2] == -1.0, "signs");
    // a segment named twice is evaluated once, the chain order kept
    a.q.n_chain = 4;
    a.q.chain_segment[3] = 1; a.q.chain_sign[3] = 1;
    frm_reduce_chain(a, ctx_seg);
    CHECK(a.n_useg == 3 && a.chain.useg[3] == 1 && a.chain.sign[3] == 1.0, "repeated segment: n_useg = %d", a.n_useg);
    a.q.n_chain = 0;
    a.q.n_params = 1;
    frm_needs(a);
    frm_reduce_chain(a, ctx_seg);
    CHECK(a.n_useg == 0 && a.chain.n_chain == 0 && a.need == (REP_NEED_R | FRM_NEED_ELEMENTS), "the centre itself: %d %d", a.n_useg, a.need);
}

struct Seg { double init, interval; int n_rec, n_coef; std::vector<double> rec; };
struct Target { double mu; int n_chain, seg[4], sign[4]; };
struct Case { int target; double et, rv[6]; };

static double rd(FILE *f) {
    double v = 0.0;
    if (std::fscanf(f, "%la", &v) != 1) { std::printf("FAIL: short input\n"); std::exit(2); }
    return v;
}
static long long ri(FILE *f) {
    long long v = 0;
    if (std::fscanf(f, "%lld", &v) != 1) { std::printf("FAIL: short input\n"); std::exit(2); }
    return v;
}

static void evaluate(const char *path) {
    FILE *f = std::fopen(path, "r");
    if (!f) { std::printf("FAIL: cannot read %s\n", path); std::exit(2); }
    const int n_seg = (int)ri(f);
    CHECK(n_seg >= 1 && n_seg <= DEV_MAX_SEG, "n_seg = %d", n_seg);
    if (n_seg < 1 || n_seg > DEV_MAX_SEG) std::exit(2);
    std::vector<Seg> segs((size_t)n_seg);
    for (Seg &s : segs) {
        s.init = rd(f); s.interval = rd(f); s.n_rec = (int)ri(f); s.n_coef = (int)ri(f);
        if (s.n_rec < 1 || s.n_coef < 1 || s.n_coef > 16) { std::printf("FAIL: segment shape\n"); std::exit(2); }
        s.rec.resize((size_t)s.n_rec * (size_t)(2 + 3 * s.n_coef));
        for (double &v : s.rec) v = rd(f);
    }
    const int n_targets = (int)ri(f);
    if (n_targets < 1 || n_targets > 64) { std::printf("FAIL: n_targets\n"); std::exit(2); }
    std::vector<Target> targets((size_t)n_targets);
    for (Target &b : targets) {
        b.mu = rd(f); b.n_chain = (int)ri(f);
        if (b.n_chain < 0 || b.n_chain > NYX_HIP_MAX_CHAIN) { std::printf("FAIL: n_chain\n"); std::exit(2); }
        for (int k = 0; k < b.n_chain; ++k) {
            b.seg[k] = (int)ri(f); b.sign[k] = (int)ri(f);
            if (b.seg[k] < 0 || b.seg[k] >= n_seg) { std::printf("FAIL: chain segment\n"); std::exit(2); }
        }
    }
    const int n_cases = (int)ri(f);
    if (n_cases < 0 || n_cases > 100000) { std::printf("FAIL: n_cases\n"); std::exit(2); }
    std::vector<Case> cases((size_t)n_cases);
    for (Case &c : cases) {
        c.target = (int)ri(f);
        if (c.target < 0 || c.target >= n_targets) { std::printf("FAIL: target\n"); std::exit(2); }
        c.et = rd(f);
        for (double &v : c.rv) v = rd(f);
    }
    std::fclose(f);

    for (int layout = 0; layout < 2; ++layout) {
        // the records as ctx_build.h lays them out: packed, or sixteen coefficients wide with zeros behind the segment's own
        DevSeg ctx_seg[DEV_MAX_SEG];
        std::memset(ctx_seg, 0, sizeof ctx_seg);
        std::vector<double> records;
        for (int i = 0; i < n_seg; ++i) {
            const Seg &s = segs[i];
            DevSeg &d = ctx_seg[i];
            d.init_et = s.init; d.interval = s.interval; d.n_rec = s.n_rec; d.n_coef = s.n_coef;
            d.end_et = s.init + s.interval * (double)s.n_rec;
            d.offset = (int32_t)records.size();
            const int src_stride = 2 + 3 * s.n_coef;
            if (layout == 1 && s.n_coef < 16) {
                d.stride = 50;
                for (int r = 0; r < s.n_rec; ++r) {
                    const double *src = s.rec.data() + (size_t)r * src_stride;
                    records.push_back(src[0]); records.push_back(src[1]);
                    for (int c = 0; c < 3; ++c)
                        for (int j = 0; j < 16; ++j) records.push_back(j < s.n_coef ? src[2 + c * s.n_coef + j] : 0.0);
                }
            } else {
                d.stride = src_stride;
                records.insert(records.end(), s.rec.begin(), s.rec.end());
            }
        }
        for (int c = 0; c < n_cases; ++c) {
            const Target &tg = targets[cases[c].target];
            FrmArgs a;
            std::memset(&a, 0, sizeof a);
            a.q = good_query();
            a.q.n_chain = tg.n_chain;
            a.q.mu_km3_s2 = tg.mu;
            for (int k = 0; k < tg.n_chain; ++k) { a.q.chain_segment[k] = tg.seg[k]; a.q.chain_sign[k] = tg.sign[k]; }
            a.q.n_params = NYX_HIP_MAX_FRAME_PARAMS;
            frm_reduce_chain(a, ctx_seg);
            // the kernel's second pass, step by step: every distinct segment once, the chain in chain order, rv' = rv - body
            for (int with_v = 1; with_v >= 0; --with_v) {
                double segpv[FRM_MAX_USEG][6];
                int st = NYX_HIP_OK;
                for (int u = 0; u < a.n_useg; ++u) {
                    double p[3], pv[3] = {0.0, 0.0, 0.0};
                    const int s1 = frm_cheby_pv(a.seg[u], records.data(), cases[c].et, with_v != 0, p, pv);
                    if (s1) st = s1;
                    for (int k = 0; k < 3; ++k) { segpv[u][k] = p[k]; segpv[u][3 + k] = pv[k]; }
                }
                double b[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
                for (int k = 0; k < a.chain.n_chain; ++k)
                    for (int i = 0; i < 6; ++i) b[i] = b[i] + a.chain.sign[k] * segpv[a.chain.useg[k]][i];
                if (!with_v) {
                    std::printf("slim %d %d %a %a %a %d\n", layout, c, b[0], b[1], b[2], st);
                    continue;
                }
                std::printf("body %d %d %a %a %a %a %a %a %d\n", layout, c, b[0], b[1], b[2], b[3], b[4], b[5], st);
                double y[6];
                for (int i = 0; i < 6; ++i) y[i] = cases[c].rv[i] - b[i];
                int32_t need = 0;
                for (int p = 0; p < NYX_HIP_FRM_COUNT; ++p) need |= frm_param_needs(p);
                FrmShared sh;
                std::memset(&sh, 0, sizeof sh);
                frm_shared(need, tg.mu, y, sh);
                for (int p = 0; p < NYX_HIP_FRM_COUNT; ++p)
                    std::printf("val %d %d %d %a %a\n", layout, c, p, frm_param(p, tg.mu, y, sh), frm_value(p, y, tg.mu));
            }
        }
    }
}

int main(int argc, char **argv) {
    refusals();
    reduction();
    if (argc > 1) evaluate(argv[1]);
    if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
    std::printf("ok\n");
    return 0;
}
