// Stand-alone check of the host side of the link report (nyx_amd/csrc/series_host.h: check_link_series, check_link_context;
// nyx_amd/csrc/link_args.h: lnk_param_needs, lnk_needs, lnk_reduce_chains) and of the kernel's own per-sample code compiled FOR THE
// HOST (nyx_amd/csrc/link_dev.h: lnk_segments, lnk_sight, lnk_sample) - g++ only, no HIP, no GPU (tests/test_link_host_cxx.py, which
// builds it plain and with the address and undefined-behaviour sanitizers).
//   link_host_check INPUT
// runs the refusals over a table of cases and the chain reduction over hand-made chains, then reads INPUT (text, numbers as
// hexadecimal floats so that every bit arrives):
//   n_seg, then per segment: init_et interval n_rec n_coef and its n_rec * (2 + 3 n_coef) record doubles
//   n_bodies, then per body: radius n_chain and n_chain pairs (segment sign)
//   n_cases, then per case: et_s, the receiver's x y z vx vy vz, the transmitter's
// lays the records out twice as the context builder may (layout 0: packed, stride 2 + 3 n_coef; layout 1: sixteen coefficients wide,
// zero-padded, stride 50) and prints per layout and case, walking the kernel's second pass with two queries of eight parameters (the
// ten of the whole link; then LosY, LosZ and the two per-body ones of the first three bodies):
//   val LAYOUT CASE PARAM BODY value status    (%a; BODY -1 for a parameter of the whole link)
// "ok" last.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../nyx_amd/csrc/link_dev.h"
#include "../../nyx_amd/csrc/series_host.h"

static int g_fail = 0;
#define CHECK(cond, ...)                                                              \
    do {                                                                              \
        if (!(cond)) {                                                                \
            if (++g_fail <= 30) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                             \
    } while (0)

static const int kSeg = 5;   // segments of the pretended context

// the centre, the Moon (+moon -earth) and the Sun (+sun -emb -earth) of an Earth-centred almanac
static nyx_hip_link_query_t good_query() {
    nyx_hip_link_query_t q;
    std::memset(&q, 0, sizeof q);
    q.n_params = 3;
    q.param[0] = NYX_HIP_LNK_RANGE;
    q.param[1] = NYX_HIP_LNK_VISIBLE;
    q.param[2] = NYX_HIP_LNK_BODY_CLEARANCE;
    q.param_body[2] = 1;
    q.step_ns = 1000000000LL;
    q.n_bodies = 3;
    q.bodies[0].n_chain = 0;
    q.bodies[0].mean_radius_km = 6378.14;
    q.bodies[1].n_chain = 2;
    q.bodies[1].chain_segment[0] = 3; q.bodies[1].chain_sign[0] = 1;
    q.bodies[1].chain_segment[1] = 0; q.bodies[1].chain_sign[1] = -1;
    q.bodies[1].mean_radius_km = 1737.4;
    q.bodies[2].n_chain = 3;
    q.bodies[2].chain_segment[0] = 2; q.bodies[2].chain_sign[0] = 1;
    q.bodies[2].chain_segment[1] = 1; q.bodies[2].chain_sign[1] = -1;
    q.bodies[2].chain_segment[2] = 0; q.bodies[2].chain_sign[2] = -1;
    q.bodies[2].mean_radius_km = 696000.0;
    return q;
}

// `why` empty: accepted; else refused with `rc` and a message that holds `why`
static void expect(const char *label, const nyx_hip_ctx *ctx, bool swapped, const nyx_hip_traj_t *t, int64_t n, const nyx_hip_traj_t *ref, int64_t n_ref,
                   const nyx_hip_link_query_t *q, int64_t capacity, const double *values, const int32_t *len, const char *why,
                   int rc = NYX_HIP_RC_BAD_ARG) {
    // (as abi.cpp chains them: the query alone, then what it asks of the context)
    Refusal r = check_link_series(ctx, t, n, ref, n_ref, q, capacity, values, len);
    if (!r) r = check_link_context(*q, kSeg, swapped);
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
    nyx_hip_link_query_t q = good_query();
    expect("good", ctx, false, &t, 1, &t, 1, &q, 4, values, len, "");
    expect("n = 0", ctx, false, &t, 0, &t, 1, &q, 4, values, len, "");
    expect("pairwise", ctx, false, &t, 7, &t, 7, &q, 4, values, len, "");
    expect("null ctx", nullptr, false, &t, 1, &t, 1, &q, 4, values, len, "null ctx");
    nyx_hip_traj_t bad_t = t;
    bad_t.len = nullptr;
    expect("null array", ctx, false, &bad_t, 1, &t, 1, &q, 4, values, len, "traj: null array");
    expect("null array of the transmitter", ctx, false, &t, 1, &bad_t, 1, &q, 4, values, len, "ref: null array");
    expect("null transmitter", ctx, false, &t, 1, nullptr, 1, &q, 4, values, len, "ref: null array");
    expect("null query", ctx, false, &t, 1, &t, 1, nullptr, 4, values, len, "traj_link: null query");
    expect("negative n", ctx, false, &t, -1, &t, 1, &q, 4, values, len, "negative n");
    expect("n_ref 2 of 7", ctx, false, &t, 7, &t, 2, &q, 4, values, len, "n_ref = 2, one transmitter trajectory or one per run (n = 7)");
    expect("n_ref 0", ctx, false, &t, 7, &t, 0, &q, 4, values, len, "n_ref = 0");
#define CASE(label, mutate, cap, why) do { q = good_query(); mutate; expect(label, ctx, false, &t, 1, &t, 1, &q, cap, values, len, why); } while (0)
    CASE("no parameter", q.n_params = 0, 4, "n_params = 0, 1 .. 8");
    CASE("nine parameters", q.n_params = 9, 4, "n_params = 9, 1 .. 8");
    CASE("unknown parameter", q.param[1] = NYX_HIP_LNK_COUNT, 4, "param[1] = 12 is not a nyx_hip_link_param");
    CASE("negative parameter", q.param[0] = -1, 4, "param[0] = -1");
    CASE("step 0", q.step_ns = 0, 4, "step_ns must be > 0");
    CASE("capacity 0", (void)0, 0, "capacity must be 1 .. 2^31 - 1");
    CASE("capacity 2^31", (void)0, (int64_t)INT32_MAX + 1, "capacity must be 1 .. 2^31 - 1");
    CASE("no body", (q.n_bodies = 0, q.n_params = 2), 4, "");
    CASE("bodies -1", q.n_bodies = -1, 4, "n_bodies = -1, 0 .. 8");
    CASE("bodies 9", q.n_bodies = 9, 4, "n_bodies = 9, 0 .. 8");
    CASE("chain -1", q.bodies[1].n_chain = -1, 4, "bodies[1].n_chain = -1, 0 .. 4");
    CASE("chain 5", q.bodies[2].n_chain = 5, 4, "bodies[2].n_chain = 5, 0 .. 4");
    CASE("segment -1", q.bodies[1].chain_segment[0] = -1, 4, "bodies[1].chain_segment[0] = -1 is not a segment of the context");
    CASE("segment of the context", q.bodies[2].chain_segment[1] = kSeg, 4, "bodies[2].chain_segment[1] = 5 is not a segment of the context (0 .. 4)");
    CASE("sign 0", q.bodies[2].chain_sign[2] = 0, 4, "bodies[2].chain_sign[2] = 0, +1 or -1");
    CASE("sign 2", q.bodies[1].chain_sign[1] = 2, 4, "bodies[1].chain_sign[1] = 2, +1 or -1");
    CASE("a bad link beyond n_chain is not read", (q.bodies[1].chain_segment[3] = 99, q.bodies[1].chain_sign[3] = 7), 4, "");
    CASE("a bad body beyond n_bodies is not read", (q.bodies[3].n_chain = 9, q.bodies[3].mean_radius_km = -1.0), 4, "");
    CASE("radius 0", q.bodies[0].mean_radius_km = 0.0, 4, "bodies[0].mean_radius_km must be finite and > 0");
    CASE("radius < 0", q.bodies[1].mean_radius_km = -1.0, 4, "bodies[1].mean_radius_km must be finite and > 0");
    CASE("radius inf", q.bodies[2].mean_radius_km = inf, 4, "bodies[2].mean_radius_km must be finite and > 0");
    CASE("radius NaN", q.bodies[0].mean_radius_km = nan, 4, "bodies[0].mean_radius_km must be finite and > 0");
    CASE("param_body 3 of 3", q.param_body[2] = 3, 4, "param_body[2] = 3, param[2] is a per-body parameter of bodies[0 .. 2]");
    CASE("param_body -1", q.param_body[2] = -1, 4, "param_body[2] = -1");
    CASE("param_body of a whole-link parameter is not read", q.param_body[0] = 77, 4, "");
    CASE("a per-body parameter without bodies", q.n_bodies = 0, 4, "param[2] is a per-body parameter and the query names no body");
    // which check wins: n_ref before the parameters, the parameters before the step, the step before the bodies, a body before
    // param_body, the query before the context
    q = good_query();
    q.n_params = 0;
    expect("n_ref before parameters", ctx, false, &t, 7, &t, 3, &q, 4, values, len, "n_ref = 3");
    CASE("parameters before step", (q.n_params = 0, q.step_ns = 0), 4, "n_params");
    CASE("step before bodies", (q.step_ns = 0, q.n_bodies = 9), 4, "step_ns");
    CASE("capacity before bodies", q.n_bodies = 9, 0, "capacity");
    CASE("a body before param_body", (q.bodies[1].chain_sign[0] = 0, q.param_body[2] = 9), 4, "chain_sign[0]");
    CASE("the query before the context", (q.bodies[1].chain_segment[0] = kSeg, q.param_body[2] = 9), 4, "param_body[2] = 9");
    q = good_query();
    expect("null values", ctx, false, &t, 1, &t, 1, &q, 4, nullptr, len, "values and len arrays required");
    expect("null len", ctx, false, &t, 1, &t, 1, &q, 4, values, nullptr, "values and len arrays required");
    q.bodies[2].chain_segment[2] = kSeg;
    expect("outputs before the context", ctx, false, &t, 1, &t, 1, &q, 4, nullptr, len, "values and len arrays required");
    expect("segments before the swap", ctx, true, &t, 1, &t, 1, &q, 4, values, len, "bodies[2].chain_segment[2] = 5");
    q = good_query();
    // the integration-frame swap: the one refusal that is not a bad argument, and the last to fire
    expect("frame swap", ctx, true, &t, 1, &t, 1, &q, 4, values, len, "integration-frame swap", NYX_HIP_RC_UNSUPPORTED);
    expect("frame swap, its wording", ctx, true, &t, 1, &t, 1, &q, 4, values, len, "a link series of them is not defined", NYX_HIP_RC_UNSUPPORTED);
    q.n_params = 0;
    expect("bad argument before the swap", ctx, true, &t, 1, &t, 1, &q, 4, values, len, "n_params");

    // ---- what each parameter needs
    CHECK(lnk_param_needs(NYX_HIP_LNK_RANGE) == LNK_NEED_RHO && lnk_param_needs(NYX_HIP_LNK_REFERENCE_DOPPLER) == LNK_NEED_RHO, "range");
    for (int p : {NYX_HIP_LNK_LOS_X, NYX_HIP_LNK_LOS_Y, NYX_HIP_LNK_LOS_Z}) CHECK(lnk_param_needs(p) == LNK_NEED_RHO, "needs of %d", p);
    CHECK(lnk_param_needs(NYX_HIP_LNK_RANGE_RATE) == (LNK_NEED_RHO | LNK_NEED_DV) && lnk_param_needs(NYX_HIP_LNK_RELATIVE_SPEED) == LNK_NEED_DV, "rates");
    for (int p : {NYX_HIP_LNK_VISIBLE, NYX_HIP_LNK_OBSTRUCTING_BODY, NYX_HIP_LNK_CLEARANCE}) CHECK(lnk_param_needs(p) == LNK_NEED_SIGHT, "needs of %d", p);
    for (int p : {NYX_HIP_LNK_BODY_CLEARANCE, NYX_HIP_LNK_BODY_OBSTRUCTS}) CHECK(lnk_param_needs(p) == LNK_NEED_BODY && lnk_param_per_body(p), "needs of %d", p);
    for (int p = 0; p < NYX_HIP_LNK_BODY_CLEARANCE; ++p) CHECK(!lnk_param_per_body(p) && lnk_param_needs(p) > 0, "needs of %d", p);
    CHECK(lnk_param_needs(NYX_HIP_LNK_COUNT) == -1 && lnk_param_needs(-1) == -1 && !lnk_param_per_body(NYX_HIP_LNK_COUNT), "needs");
    CHECK(NYX_HIP_LNK_COUNT == 12 && sizeof(LnkArgs) <= 4096, "the enum and the argument block");
}

static void reduction() {
    DevSeg ctx_seg[DEV_MAX_SEG];
    std::memset(ctx_seg, 0, sizeof ctx_seg);
    for (int k = 0; k < DEV_MAX_SEG; ++k) ctx_seg[k].offset = 1000 + k;   // (a tag: which row was copied)
    LnkArgs a;
    std::memset(&a, 0, sizeof a);
    a.q = good_query();
    lnk_needs(a);
    CHECK(a.need == (LNK_NEED_RHO | LNK_NEED_SIGHT | LNK_NEED_BODY) && a.body_mask == 2, "need %d mask %d", a.need, a.body_mask);
    CHECK(lnk_reduce_chains(a, ctx_seg), "reduce");
    // the Moon names 3 and 0, the Sun 2, 1 and 0 again: four distinct segments, first use first
    CHECK(a.n_useg == 4, "n_useg = %d", a.n_useg);
    const int want_index[4] = {3, 0, 2, 1};
    for (int u = 0; u < 4; ++u) CHECK(a.seg_index[u] == want_index[u] && a.seg[u].offset == 1000 + want_index[u], "useg %d = %d", u, a.seg_index[u]);
    CHECK(a.body[0].n_chain == 0 && a.body[0].radius_km == 6378.14, "the centre");
    CHECK(a.body[1].n_chain == 2 && a.body[1].useg[0] == 0 && a.body[1].useg[1] == 1 && a.body[1].sign[0] == 1.0 && a.body[1].sign[1] == -1.0, "the Moon");
    CHECK(a.body[2].n_chain == 3 && a.body[2].useg[0] == 2 && a.body[2].useg[1] == 3 && a.body[2].useg[2] == 1 && a.body[2].sign[2] == -1.0 &&
              a.body[2].radius_km == 696000.0, "the Sun");
    // the default - the centre alone - evaluates no segment at all
    a.q.n_bodies = 1;
    a.q.n_params = 2;
    lnk_needs(a);
    CHECK(lnk_reduce_chains(a, ctx_seg) && a.n_useg == 0 && a.need == (LNK_NEED_RHO | LNK_NEED_SIGHT) && a.body_mask == 0, "the centre alone: %d", a.n_useg);
    a.q.n_bodies = 0;
    CHECK(lnk_reduce_chains(a, ctx_seg) && a.n_useg == 0, "no body");
    // the eclipses reduce as before through the shared step: the light source first, then the bodies
    EclArgs e;
    std::memset(&e, 0, sizeof e);
    e.q.light = good_query().bodies[2];
    e.q.n_bodies = 2;
    e.q.bodies[0] = good_query().bodies[0];
    e.q.bodies[1] = good_query().bodies[1];
    CHECK(ecl_reduce_chains(e, ctx_seg) && e.n_useg == 4, "eclipse n_useg = %d", e.n_useg);
    const int ecl_index[4] = {2, 1, 0, 3};
    for (int u = 0; u < 4; ++u) CHECK(e.seg_index[u] == ecl_index[u] && e.seg[u].offset == 1000 + ecl_index[u], "eclipse useg %d = %d", u, e.seg_index[u]);
    CHECK(e.light.n_chain == 3 && e.light.useg[2] == 2 && e.body[1].useg[0] == 3 && e.body[1].useg[1] == 2 && e.body[0].n_chain == 0, "eclipse chains");
    // more distinct segments than a context holds: refused, not overrun
    nyx_hip_link_query_t many = good_query();
    many.n_bodies = 3;
    for (int b = 0; b < 3; ++b) {
        many.bodies[b].n_chain = 4;
        for (int k = 0; k < 4; ++k) { many.bodies[b].chain_segment[k] = 4 * b + k; many.bodies[b].chain_sign[k] = 1; }
    }
    a.q = many;
    DevSeg wide[16];
    std::memset(wide, 0, sizeof wide);
    CHECK(!lnk_reduce_chains(a, wide) && a.n_useg == ECL_MAX_USEG, "nine distinct segments: n_useg = %d", a.n_useg);
}

struct Seg { double init, interval; int n_rec, n_coef; std::vector<double> rec; };
struct Body { double radius; int n_chain, seg[4], sign[4]; };
struct Case { double et, rx[6], tx[6]; };

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
    if (n_seg < 1 || n_seg > DEV_MAX_SEG) { std::printf("FAIL: n_seg\n"); std::exit(2); }
    std::vector<Seg> segs((size_t)n_seg);
    for (Seg &s : segs) {
        s.init = rd(f); s.interval = rd(f); s.n_rec = (int)ri(f); s.n_coef = (int)ri(f);
        if (s.n_rec < 1 || s.n_coef < 1 || s.n_coef > 16) { std::printf("FAIL: segment shape\n"); std::exit(2); }
        s.rec.resize((size_t)s.n_rec * (size_t)(2 + 3 * s.n_coef));
        for (double &v : s.rec) v = rd(f);
    }
    const int n_bodies = (int)ri(f);
    if (n_bodies < 3 || n_bodies > NYX_HIP_MAX_LINK_BODIES) { std::printf("FAIL: n_bodies\n"); std::exit(2); }
    std::vector<Body> bodies((size_t)n_bodies);
    for (Body &b : bodies) {
        b.radius = rd(f); b.n_chain = (int)ri(f);
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
        c.et = rd(f);
        for (double &v : c.rx) v = rd(f);
        for (double &v : c.tx) v = rd(f);
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
        for (int group = 0; group < 2; ++group) {
            LnkArgs a;
            std::memset(&a, 0, sizeof a);
            a.q.step_ns = 1;
            a.q.n_bodies = n_bodies;
            for (int b = 0; b < n_bodies; ++b) {
                a.q.bodies[b].n_chain = bodies[b].n_chain;
                a.q.bodies[b].mean_radius_km = bodies[b].radius;
                for (int k = 0; k < bodies[b].n_chain; ++k) { a.q.bodies[b].chain_segment[k] = bodies[b].seg[k]; a.q.bodies[b].chain_sign[k] = bodies[b].sign[k]; }
            }
            a.q.n_params = NYX_HIP_MAX_LINK_PARAMS;
            for (int p = 0; p < 8; ++p) {
                if (group == 0) { a.q.param[p] = p; continue; }
                if (p < 2) { a.q.param[p] = NYX_HIP_LNK_LOS_Y + p; continue; }
                a.q.param[p] = (p - 2) % 2 ? NYX_HIP_LNK_BODY_OBSTRUCTS : NYX_HIP_LNK_BODY_CLEARANCE;
                a.q.param_body[p] = (p - 2) / 2;
            }
            a.records = records.data();
            lnk_needs(a);
            if (!lnk_reduce_chains(a, ctx_seg)) { std::printf("FAIL: reduction\n"); std::exit(2); }
            for (int c = 0; c < n_cases; ++c) {
                // the kernel's second pass: every distinct segment once, then the sample
                double segpos[ECL_MAX_USEG][3];
                std::memset(segpos, 0, sizeof segpos);
                const int st = lnk_segments(a, cases[c].et, &segpos[0][0], 3, 1);
                int written = 0;
                lnk_sample(a, cases[c].rx, cases[c].tx, &segpos[0][0], 3, 1, [&](int p, double val) {
                    ++written;
                    std::printf("val %d %d %d %d %a %d\n", layout, c, a.q.param[p], lnk_param_per_body(a.q.param[p]) ? a.q.param_body[p] : -1, val, st);
                });
                CHECK(written == a.q.n_params, "case %d: %d values of %d", c, written, a.q.n_params);
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
