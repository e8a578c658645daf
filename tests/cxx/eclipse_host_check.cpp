// Stand-alone check of the host side of the eclipse report (nyx_amd/csrc/series_host.h: check_ecl_series; nyx_amd/csrc/eclipse_args.h:
// ecl_param_needs, ecl_needs, ecl_reduce_chains) and of the kernel's own per-sample code compiled FOR THE HOST
// (nyx_amd/csrc/chain_dev.h: frm_cheby_pv; nyx_amd/csrc/eclipse_dev.h: ecl_occultation) - g++ only, no HIP, no GPU (tests/test_eclipse_host_cxx.py, which builds
// it with the address and undefined-behaviour sanitizers).
//   eclipse_host_check INPUT
// runs check_ecl_series over a table of cases and the chain reduction over hand-made chains, then reads INPUT (text, numbers as
// hexadecimal floats so that every bit arrives):
//   n_seg, then per segment: init_et interval n_rec n_coef and its n_rec * (2 + 3 n_coef) record doubles
//   n_bodies (the light source first), then per body: radius n_chain and n_chain pairs (segment sign)
//   n_cases, then per case: epoch_ns (0 <= ns < one century) x y z
// lays the records out twice as the context builder may (layout 0: packed, stride 2 + 3 n_coef; layout 1: sixteen coefficients wide,
// zero-padded, stride 50), reduces the chains to their distinct segments, and prints per layout and case, walking the kernel's steps:
//   pos LAYOUT CASE BODY x y z status            the chain summed in chain order (%a)
//   pct LAYOUT CASE BODY pct factor branch       of body >= 1 against the light source; factor = pct / 100
// "ok" last.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <limits>
#include <vector>

#include "../../nyx_amd/csrc/eclipse_dev.h"
#include "../../nyx_amd/csrc/series_host.h"

static int g_fail = 0;
#define CHECK(cond, ...)                                                              \
    do {                                                                              \
        if (!(cond)) {                                                                \
            if (++g_fail <= 30) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                             \
    } while (0)

static const int kSeg = 5;   // segments of the pretended context

static nyx_hip_ecl_body_t body(double radius, int n_chain, int s0 = 0, int g0 = 1, int s1 = 0, int g1 = 1, int s2 = 0, int g2 = 1) {
    nyx_hip_ecl_body_t b;
    std::memset(&b, 0, sizeof b);
    b.n_chain = n_chain;
    b.chain_segment[0] = s0; b.chain_sign[0] = g0;
    b.chain_segment[1] = s1; b.chain_sign[1] = g1;
    b.chain_segment[2] = s2; b.chain_sign[2] = g2;
    b.chain_sign[3] = 1;
    b.mean_radius_km = radius;
    return b;
}

// the cislunar model of an Earth-centred almanac: Sun = +sun - emb - earth, Earth the centre, Moon = +moon - earth
static nyx_hip_ecl_query_t good_query() {
    nyx_hip_ecl_query_t q;
    std::memset(&q, 0, sizeof q);
    q.n_params = 3;
    q.param[0] = NYX_HIP_ECL_OCCULTATION;
    q.param[1] = NYX_HIP_ECL_STATE;
    q.param[2] = NYX_HIP_ECL_BODY_PENUMBRA_MARGIN;
    q.param_body[2] = 1;
    q.step_ns = 1000000000LL;
    q.light = body(696000.0, 3, 2, 1, 1, -1, 0, -1);
    q.n_bodies = 2;
    q.bodies[0] = body(6378.1363, 0);
    q.bodies[1] = body(1737.4, 2, 3, 1, 0, -1);
    return q;
}

// `why` empty: accepted; else refused with `rc` and a message that holds `why`
static void expect(const char *label, const nyx_hip_ctx *ctx, bool swapped, const nyx_hip_traj_t *t, int64_t n, const nyx_hip_ecl_query_t *q,
                   int64_t capacity, const double *values, const int32_t *len, const char *why, int rc = NYX_HIP_RC_BAD_ARG) {
    // (as abi.cpp chains them: the query alone, then what it asks of the context)
    Refusal r = check_ecl_series(ctx, t, n, q, capacity, values, len);
    if (!r) r = check_ecl_context(*q, kSeg, swapped);
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
    double values[1];
    int32_t len[1];
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    nyx_hip_ecl_query_t q = good_query();
    expect("good", ctx, false, &t, 1, &q, 4, values, len, "");
    expect("n = 0", ctx, false, &t, 0, &q, 4, values, len, "");
    expect("null ctx", nullptr, false, &t, 1, &q, 4, values, len, "null ctx");
    nyx_hip_traj_t bad_t = t;
    bad_t.len = nullptr;
    expect("null array", ctx, false, &bad_t, 1, &q, 4, values, len, "traj: null array");
    expect("null query", ctx, false, &t, 1, nullptr, 4, values, len, "traj_eclipse: null query");
    expect("negative n", ctx, false, &t, -1, &q, 4, values, len, "negative n");
#define CASE(label, mutate, cap, why) do { q = good_query(); mutate; expect(label, ctx, false, &t, 1, &q, cap, values, len, why); } while (0)
    CASE("no parameter", q.n_params = 0, 4, "n_params = 0, 1 .. 8");
    CASE("nine parameters", q.n_params = 9, 4, "n_params = 9, 1 .. 8");
    CASE("unknown parameter", q.param[1] = NYX_HIP_ECL_COUNT, 4, "param[1] = 11 is not a nyx_hip_ecl_param");
    CASE("negative parameter", q.param[0] = -1, 4, "param[0] = -1");
    CASE("step 0", q.step_ns = 0, 4, "step_ns must be > 0");
    CASE("capacity 0", (void)0, 0, "capacity must be 1 .. 2^31 - 1");
    CASE("capacity 2^31", (void)0, (int64_t)INT32_MAX + 1, "capacity must be 1 .. 2^31 - 1");
    CASE("no body", q.n_bodies = 0, 4, "n_bodies = 0, 1 .. 8");
    CASE("nine bodies", q.n_bodies = 9, 4, "n_bodies = 9, 1 .. 8");
    CASE("eight bodies", (q.n_bodies = 8, q.bodies[2] = q.bodies[3] = q.bodies[4] = q.bodies[5] = q.bodies[6] = q.bodies[7] = q.bodies[1]), 4, "");
    CASE("light at the centre", q.light.n_chain = 0, 4, "light.n_chain = 0, 1 .. 4");
    CASE("light chain 5", q.light.n_chain = 5, 4, "light.n_chain = 5, 1 .. 4");
    CASE("light segment", q.light.chain_segment[1] = kSeg, 4, "light.chain_segment[1] = 5 is not a segment of the context (0 .. 4)");
    CASE("light segment -1", q.light.chain_segment[0] = -1, 4, "light.chain_segment[0] = -1");
    CASE("light sign 0", q.light.chain_sign[2] = 0, 4, "light.chain_sign[2] = 0, +1 or -1");
    CASE("light radius 0", q.light.mean_radius_km = 0.0, 4, "light.mean_radius_km must be finite and > 0");
    CASE("light radius inf", q.light.mean_radius_km = inf, 4, "light.mean_radius_km must be finite and > 0");
    CASE("body chain -1", q.bodies[0].n_chain = -1, 4, "bodies[0].n_chain = -1, 0 .. 4");
    CASE("body chain 5", q.bodies[1].n_chain = 5, 4, "bodies[1].n_chain = 5, 0 .. 4");
    CASE("body chain 4", (q.bodies[1].n_chain = 4, q.bodies[1].chain_segment[3] = 4), 4, "");
    CASE("body segment", q.bodies[1].chain_segment[0] = 7, 4, "bodies[1].chain_segment[0] = 7 is not a segment of the context");
    CASE("body sign 2", q.bodies[1].chain_sign[1] = 2, 4, "bodies[1].chain_sign[1] = 2, +1 or -1");
    CASE("body radius NaN", q.bodies[0].mean_radius_km = nan, 4, "bodies[0].mean_radius_km must be finite and > 0");
    CASE("body radius < 0", q.bodies[1].mean_radius_km = -1.0, 4, "bodies[1].mean_radius_km must be finite and > 0");
    CASE("a bad body beyond n_bodies is not read", q.bodies[2].n_chain = 9, 4, "");
    CASE("a bad segment beyond n_chain is not read", q.bodies[1].chain_segment[2] = 99, 4, "");
    CASE("param_body 2", q.param_body[2] = 2, 4, "param_body[2] = 2, param[2] is a per-body parameter of bodies[0 .. 1]");
    CASE("param_body -1", q.param_body[2] = -1, 4, "param_body[2] = -1");
    CASE("param_body of a model parameter is not read", q.param_body[0] = 99, 4, "");
    // which check wins: the parameters before the step, the step before the bodies, the light before the bodies, the bodies before param_body
    CASE("parameters before step", (q.n_params = 0, q.step_ns = 0), 4, "n_params");
    CASE("step before bodies", (q.step_ns = 0, q.n_bodies = 0), 4, "step_ns");
    CASE("count before light", (q.n_bodies = 0, q.light.n_chain = 0), 4, "n_bodies");
    CASE("light before bodies", (q.light.n_chain = 0, q.bodies[0].n_chain = 9), 4, "light.n_chain");
    CASE("bodies before param_body", (q.bodies[1].chain_sign[0] = 0, q.param_body[2] = 5), 4, "bodies[1].chain_sign[0]");
    CASE("the query before the context", (q.light.chain_segment[0] = kSeg, q.param_body[2] = 5), 4, "param_body[2]");
    q = good_query();
    expect("null values", ctx, false, &t, 1, &q, 4, nullptr, len, "values and len arrays required");
    expect("null len", ctx, false, &t, 1, &q, 4, values, nullptr, "values and len arrays required");
    q.bodies[1].chain_segment[1] = kSeg;
    expect("outputs before the context", ctx, false, &t, 1, &q, 4, nullptr, len, "values and len arrays required");
    expect("segment of the context", ctx, false, &t, 1, &q, 4, values, len, "bodies[1].chain_segment[1] = 5 is not a segment of the context (0 .. 4)");
    expect("segments before the swap", ctx, true, &t, 1, &q, 4, values, len, "bodies[1].chain_segment[1] = 5");
    q = good_query();
    // the integration-frame swap: the one refusal that is not a bad argument, and the last to fire
    expect("frame swap", ctx, true, &t, 1, &q, 4, values, len, "integration-frame swap", NYX_HIP_RC_UNSUPPORTED);
    q.n_params = 0;
    expect("bad argument before the swap", ctx, true, &t, 1, &q, 4, values, len, "n_params");

    // ---- what each parameter needs
    CHECK(ecl_param_needs(NYX_HIP_ECL_SUN_RANGE) == 0 && ecl_param_needs(NYX_HIP_ECL_SUN_APPARENT_RADIUS) == ECL_NEED_SUN_RADIUS, "needs");
    for (int p : {NYX_HIP_ECL_OCCULTATION, NYX_HIP_ECL_ILLUMINATION, NYX_HIP_ECL_STATE, NYX_HIP_ECL_ECLIPSING_BODY})
        CHECK(ecl_param_needs(p) == (ECL_NEED_SUN_RADIUS | ECL_NEED_MODEL) && !ecl_param_per_body(p), "needs of %d", p);
    for (int p = NYX_HIP_ECL_BODY_OCCULTATION; p < NYX_HIP_ECL_COUNT; ++p)
        CHECK(ecl_param_needs(p) == (ECL_NEED_SUN_RADIUS | ECL_NEED_BODY) && ecl_param_per_body(p), "needs of %d", p);
    CHECK(ecl_param_needs(NYX_HIP_ECL_COUNT) == -1 && ecl_param_needs(-1) == -1 && !ecl_param_per_body(NYX_HIP_ECL_COUNT), "needs");
}

static void reduction() {
    DevSeg ctx_seg[DEV_MAX_SEG];
    std::memset(ctx_seg, 0, sizeof ctx_seg);
    for (int k = 0; k < DEV_MAX_SEG; ++k) ctx_seg[k].offset = 1000 + k;   // (a tag: which row was copied)
    EclArgs a;
    std::memset(&a, 0, sizeof a);
    a.q = good_query();
    ecl_needs(a);
    CHECK(a.need == (ECL_NEED_SUN_RADIUS | ECL_NEED_MODEL | ECL_NEED_BODY) && a.body_mask == 2, "need %d mask %d", a.need, a.body_mask);
    CHECK(ecl_reduce_chains(a, ctx_seg), "reduce");
    // Sun: segments 2, 1, 0 in chain order; the Moon's 3 is new, its 0 (Earth w.r.t. the EMB) is the Sun's third: counted once
    CHECK(a.n_useg == 4, "n_useg = %d", a.n_useg);
    const int want_index[4] = {2, 1, 0, 3};
    for (int u = 0; u < 4; ++u) CHECK(a.seg_index[u] == want_index[u] && a.seg[u].offset == 1000 + want_index[u], "useg %d = %d", u, a.seg_index[u]);
    CHECK(a.light.n_chain == 3 && a.light.useg[0] == 0 && a.light.useg[1] == 1 && a.light.useg[2] == 2, "light chain");
    CHECK(a.light.sign[0] == 1.0 && a.light.sign[1] == -1.0 && a.light.sign[2] == -1.0 && a.light.radius_km == 696000.0, "light signs");
    CHECK(a.body[0].n_chain == 0 && a.body[0].radius_km == 6378.1363, "the centre");
    CHECK(a.body[1].n_chain == 2 && a.body[1].useg[0] == 3 && a.body[1].useg[1] == 2 && a.body[1].sign[0] == 1.0 && a.body[1].sign[1] == -1.0, "moon chain");
    // only the model's parameters: no body is singled out
    a.q.n_params = 2;
    ecl_needs(a);
    CHECK(a.need == (ECL_NEED_SUN_RADIUS | ECL_NEED_MODEL) && a.body_mask == 0, "need %d mask %d", a.need, a.body_mask);
    a.q.n_params = 1;
    a.q.param[0] = NYX_HIP_ECL_SUN_RANGE;
    ecl_needs(a);
    CHECK(a.need == 0 && a.body_mask == 0, "need %d", a.need);
    // eight bodies of four segments each over the eight segments of a context: eight distinct ones, every chain kept in order
    a.q = good_query();
    a.q.n_bodies = 8;
    for (int b = 0; b < 8; ++b) {
        a.q.bodies[b] = body(10.0 + b, 4);
        for (int k = 0; k < 4; ++k) { a.q.bodies[b].chain_segment[k] = (b + 2 * k) % 8; a.q.bodies[b].chain_sign[k] = k % 2 ? -1 : 1; }
    }
    CHECK(ecl_reduce_chains(a, ctx_seg) && a.n_useg == 8, "n_useg = %d", a.n_useg);
    for (int b = 0; b < 8; ++b)
        for (int k = 0; k < 4; ++k) CHECK(a.seg_index[a.body[b].useg[k]] == (b + 2 * k) % 8 && a.body[b].sign[k] == (k % 2 ? -1.0 : 1.0), "body %d link %d", b, k);
}

struct Seg { double init, interval; int n_rec, n_coef; std::vector<double> rec; };
struct Body { double radius; int n_chain, seg[4], sign[4]; };

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
    std::vector<Seg> segs((size_t)n_seg);
    for (Seg &s : segs) {
        s.init = rd(f); s.interval = rd(f); s.n_rec = (int)ri(f); s.n_coef = (int)ri(f);
        s.rec.resize((size_t)s.n_rec * (size_t)(2 + 3 * s.n_coef));
        for (double &v : s.rec) v = rd(f);
    }
    const int n_bodies = (int)ri(f);
    CHECK(n_bodies >= 2 && n_bodies <= 1 + NYX_HIP_MAX_ECL_BODIES, "n_bodies = %d", n_bodies);
    std::vector<Body> bodies((size_t)n_bodies);
    for (Body &b : bodies) {
        b.radius = rd(f); b.n_chain = (int)ri(f);
        for (int k = 0; k < b.n_chain && k < 4; ++k) { b.seg[k] = (int)ri(f); b.sign[k] = (int)ri(f); }
    }
    const int n_cases = (int)ri(f);
    std::vector<long long> epochs((size_t)n_cases);
    std::vector<double> pos((size_t)n_cases * 3);
    for (int c = 0; c < n_cases; ++c) { epochs[c] = ri(f); for (int k = 0; k < 3; ++k) pos[3 * c + k] = rd(f); }
    std::fclose(f);

    EclArgs a;
    std::memset(&a, 0, sizeof a);
    a.q = good_query();
    a.q.n_bodies = n_bodies - 1;
    for (int b = 0; b < n_bodies; ++b) {
        nyx_hip_ecl_body_t &dst = b == 0 ? a.q.light : a.q.bodies[b - 1];
        std::memset(&dst, 0, sizeof dst);
        dst.n_chain = bodies[b].n_chain;
        dst.mean_radius_km = bodies[b].radius;
        for (int k = 0; k < bodies[b].n_chain; ++k) { dst.chain_segment[k] = bodies[b].seg[k]; dst.chain_sign[k] = bodies[b].sign[k]; }
    }
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
        CHECK(ecl_reduce_chains(a, ctx_seg), "reduce");
        for (int c = 0; c < n_cases; ++c) {
            // (0 <= ns < one century: Duration::to_seconds is whole seconds plus the sub-second part)
            const double et = (double)(epochs[c] / 1000000000LL) + (double)(epochs[c] % 1000000000LL) * 1e-9;
            const double *r = &pos[3 * c];
            // the kernel's second pass, step by step: every distinct segment once, then the chains in chain order
            double segpos[ECL_MAX_USEG][3];
            int seg_st[ECL_MAX_USEG];
            for (int u = 0; u < a.n_useg; ++u) seg_st[u] = frm_cheby_pv(a.seg[u], records.data(), et, false, segpos[u], nullptr);
            double p_body[1 + NYX_HIP_MAX_ECL_BODIES][3];
            for (int b = 0; b < n_bodies; ++b) {
                const EclChain &ch = b == 0 ? a.light : a.body[b - 1];
                double s0 = 0.0, s1 = 0.0, s2 = 0.0;
                int st = 0;
                for (int k = 0; k < ch.n_chain; ++k) {
                    s0 = s0 + ch.sign[k] * segpos[ch.useg[k]][0];
                    s1 = s1 + ch.sign[k] * segpos[ch.useg[k]][1];
                    s2 = s2 + ch.sign[k] * segpos[ch.useg[k]][2];
                    if (seg_st[ch.useg[k]]) st = seg_st[ch.useg[k]];
                }
                p_body[b][0] = s0; p_body[b][1] = s1; p_body[b][2] = s2;
                std::printf("pos %d %d %d %a %a %a %d\n", layout, c, b, s0, s1, s2, st);
            }
            const double r_ls[3] = {p_body[0][0] - r[0], p_body[0][1] - r[1], p_body[0][2] - r[2]};
            const double n_ls = ecl_norm3(r_ls);
            const double ls_p = ecl_apparent(a.light.radius_km, n_ls);
            for (int b = 1; b < n_bodies; ++b) {
                const double r_eb[3] = {r[0] - p_body[b][0], r[1] - p_body[b][1], r[2] - p_body[b][2]};
                const EclDisk d = ecl_occultation(ls_p, n_ls, a.body[b - 1].radius_km, r_eb, r_ls);
                const char *branch = d.d_p - ls_p > d.fo_p ? "lit" : d.fo_p > d.d_p + ls_p ? "umbra"
                                     : (std::fabs(ls_p - d.fo_p) < d.d_p && d.d_p < ls_p + d.fo_p) ? "penumbra" : "annular";
                std::printf("pct %d %d %d %a %a %s\n", layout, c, b, d.pct, d.pct / 100.0, branch);
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
