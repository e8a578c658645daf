// lambert_host_check.cpp — the host side of the Lambert transfers, stand-alone (its own main; g++ only, no HIP, no GPU):
// nyx_amd/csrc/lambert_args.h (what the two entries refuse, as abi.cpp chains the checks) and THE KERNELS' OWN per-problem code compiled
// for the host, nyx_amd/csrc/lambert_dev.h (the solver, the status rules, the parameters, a body's state about the centre through
// frm_cheby_pv).  Run by tests/test_lambert_host_cxx.py, plain and under the address and undefined-behaviour sanitizers.
//
// Without an argument: the refusal table, "ok" last.  With an input file (hex floats): segments, three chains, then problems
//   prob WAY N_REVS HIGH_PATH MAX_ITER TOL MU rv1[6] rv2[6] TOF   ->  "sol CASE status v[16]"                      (%a)
// and grid cells
//   cell ET_DEP ET_ARR TOF MU                                     ->  "cell LAYOUT CASE st1 rv1[6] st2 rv2[6] status v[16]"
// the records laid out twice as the context builder may (layout 0: packed; layout 1: sixteen coefficients wide, zero-padded), and the
// time of one solve on this core: "time NS_PER_SOLVE SOLVES".
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../nyx_amd/csrc/lambert_dev.h"

static int g_fail = 0;
#define CHECK(cond, ...)                                                              \
    do {                                                                              \
        if (!(cond)) {                                                                \
            if (++g_fail <= 30) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                             \
    } while (0)

#include "block_check.h"

static const int kSeg = 5;   // segments of the pretended context

static nyx_hip_lambert_query_t good_solver() {
    nyx_hip_lambert_query_t q;
    std::memset(&q, 0, sizeof q);
    q.n_params = 2;
    q.param[0] = NYX_HIP_LMB_C3;
    q.param[1] = NYX_HIP_LMB_DV_TOTAL;
    q.way = NYX_HIP_LMB_AUTO;
    q.max_iter = 1000;
    q.tol = 1e-4;
    return q;
}

// Earth -> Jupiter about the Sun in an Earth-centred almanac
static nyx_hip_lambert_grid_query_t good_grid() {
    nyx_hip_lambert_grid_query_t q;
    std::memset(&q, 0, sizeof q);
    q.solve = good_solver();
    q.dep.n_chain = 0;
    q.arr.n_chain = 3;
    q.arr.chain_segment[0] = 4; q.arr.chain_sign[0] = 1;
    q.arr.chain_segment[1] = 1; q.arr.chain_sign[1] = -1;
    q.arr.chain_segment[2] = 0; q.arr.chain_sign[2] = -1;
    q.centre.n_chain = 3;
    q.centre.chain_segment[0] = 2; q.centre.chain_sign[0] = 1;
    q.centre.chain_segment[1] = 1; q.centre.chain_sign[1] = -1;
    q.centre.chain_segment[2] = 0; q.centre.chain_sign[2] = -1;
    q.n_dep = 4; q.n_arr = 5;
    q.dep_step_ns = q.arr_step_ns = q.tof_step_ns = 1000000000LL;
    q.mu_km3_s2 = 1.32712440018e11;
    return q;
}

static void expect(const char *label, const Refusal &r, const char *why, int rc = NYX_HIP_RC_BAD_ARG) {
    if (!*why) CHECK(r.rc == NYX_HIP_RC_OK, "%s: refused with '%s'", label, r.msg);
    else CHECK(r.rc == rc && std::strstr(r.msg, why) != nullptr, "%s: rc %d, message '%s', expected %d '%s'", label, r.rc, r.msg, rc, why);
}

// (as abi.cpp chains them: the query alone, then what it asks of the context)
static Refusal grid_checks(const nyx_hip_ctx *ctx, const nyx_hip_lambert_grid_query_t *q, const double *v, const int32_t *s, bool swapped = false) {
    Refusal r = check_lambert_grid(ctx, q, v, s);
    if (!r) r = check_lambert_context(*q, kSeg, swapped);
    return r;
}

static void refusals() {
    const nyx_hip_ctx *ctx = (const nyx_hip_ctx *)(uintptr_t)1;   // never dereferenced
    double x[1] = {0};
    int32_t st[1] = {0};
    const double mu = 398600.4;
    nyx_hip_lambert_query_t q = good_solver();
    expect("batch: good", check_lambert_batch(ctx, x, x, x, 1, mu, &q, x, st), "");
    expect("batch: n = 0", check_lambert_batch(ctx, x, x, x, 0, mu, &q, x, st), "");
    expect("batch: null ctx", check_lambert_batch(nullptr, x, x, x, 1, mu, &q, x, st), "null ctx");
    expect("batch: null query", check_lambert_batch(ctx, x, x, x, 1, mu, nullptr, x, st), "lambert_batch: null query");
    struct { const char *label; void (*edit)(nyx_hip_lambert_query_t &); const char *why; } solver[] = {
        {"n_params 0", [](nyx_hip_lambert_query_t &s) { s.n_params = 0; }, "n_params = 0, 1 .. 8 parameters per call"},
        {"n_params 9", [](nyx_hip_lambert_query_t &s) { s.n_params = 9; }, "n_params = 9"},
        {"param 16", [](nyx_hip_lambert_query_t &s) { s.param[1] = 16; }, "param[1] = 16 is not a nyx_hip_lambert_param"},
        {"param -1", [](nyx_hip_lambert_query_t &s) { s.param[0] = -1; }, "param[0] = -1"},
        {"param beyond n_params", [](nyx_hip_lambert_query_t &s) { s.param[2] = 99; }, ""},
        {"way 3", [](nyx_hip_lambert_query_t &s) { s.way = 3; }, "way = 3 is not a nyx_hip_lambert_way"},
        {"n_revs -1", [](nyx_hip_lambert_query_t &s) { s.n_revs = -1; }, "n_revs = -1, 0 .. 255"},
        {"n_revs 256", [](nyx_hip_lambert_query_t &s) { s.n_revs = 256; }, "n_revs = 256"},
        {"n_revs 255", [](nyx_hip_lambert_query_t &s) { s.n_revs = 255; s.high_path = 1; }, ""},
        {"high_path 2", [](nyx_hip_lambert_query_t &s) { s.high_path = 2; }, "high_path = 2, 0 or 1"},
        {"tol small", [](nyx_hip_lambert_query_t &s) { s.tol = 9e-14; }, "1e-13 .. 1e-2"},
        {"tol large", [](nyx_hip_lambert_query_t &s) { s.tol = 0.011; }, "1e-13 .. 1e-2"},
        {"tol nan", [](nyx_hip_lambert_query_t &s) { s.tol = std::nan(""); }, "tol = nan"},
        {"tol edges", [](nyx_hip_lambert_query_t &s) { s.tol = 1e-13; }, ""},
        {"max_iter 0", [](nyx_hip_lambert_query_t &s) { s.max_iter = 0; }, "max_iter = 0, 1 .. 1000"},
        {"max_iter 1001", [](nyx_hip_lambert_query_t &s) { s.max_iter = 1001; }, "max_iter = 1001"},
        {"order: n_params first", [](nyx_hip_lambert_query_t &s) { s.n_params = 0; s.way = 9; s.tol = 1.0; }, "n_params = 0"},
        {"order: way before n_revs", [](nyx_hip_lambert_query_t &s) { s.way = 9; s.n_revs = 999; }, "way = 9"},
        {"order: tol before max_iter", [](nyx_hip_lambert_query_t &s) { s.tol = 1.0; s.max_iter = 0; }, "tol = 1"},
    };
    for (auto &c : solver) {
        nyx_hip_lambert_query_t s = good_solver();
        c.edit(s);
        expect(c.label, check_lambert_batch(ctx, x, x, x, 1, mu, &s, x, st), c.why);
        nyx_hip_lambert_grid_query_t g = good_grid();
        g.solve = s;
        expect(c.label, grid_checks(ctx, &g, x, st), c.why);
    }
    for (double bad : {0.0, -1.0, (double)NAN, (double)INFINITY}) {
        expect("batch: mu", check_lambert_batch(ctx, x, x, x, 1, bad, &q, x, st), "lambert_batch: mu_km3_s2 must be finite and > 0");
        nyx_hip_lambert_grid_query_t g = good_grid();
        g.mu_km3_s2 = bad;
        expect("grid: mu", grid_checks(ctx, &g, x, st), "lambert_grid: mu_km3_s2 must be finite and > 0");
    }
    expect("batch: mu before n", check_lambert_batch(ctx, x, x, x, -1, 0.0, &q, x, st), "mu_km3_s2");
    expect("batch: negative n", check_lambert_batch(ctx, nullptr, x, x, -1, mu, &q, x, st), "negative n");
    expect("batch: rv1", check_lambert_batch(ctx, nullptr, x, x, 1, mu, &q, nullptr, st), "rv1, rv2 and tof_s arrays required");
    expect("batch: rv2", check_lambert_batch(ctx, x, nullptr, x, 1, mu, &q, x, st), "rv1, rv2 and tof_s arrays required");
    expect("batch: tof", check_lambert_batch(ctx, x, x, nullptr, 1, mu, &q, x, st), "rv1, rv2 and tof_s arrays required");
    expect("batch: values", check_lambert_batch(ctx, x, x, x, 1, mu, &q, nullptr, st), "values and status arrays required");
    expect("batch: status", check_lambert_batch(ctx, x, x, x, 1, mu, &q, x, nullptr), "values and status arrays required");

    nyx_hip_lambert_grid_query_t g = good_grid();
    expect("grid: good", grid_checks(ctx, &g, x, st), "");
    expect("grid: null ctx", grid_checks(nullptr, &g, x, st), "null ctx");
    expect("grid: null query", check_lambert_grid(ctx, nullptr, x, st), "lambert_grid: null query");
    struct { const char *label; void (*edit)(nyx_hip_lambert_grid_query_t &); const char *why; } grid[] = {
        {"empty", [](nyx_hip_lambert_grid_query_t &c) { c.n_dep = 0; c.n_arr = 0; }, ""},
        {"n_dep -1", [](nyx_hip_lambert_grid_query_t &c) { c.n_dep = -1; }, "n_dep = -1, n_arr = 5"},
        {"n_arr -1", [](nyx_hip_lambert_grid_query_t &c) { c.n_arr = -1; }, "n_arr = -1"},
        {"n_arr 2^31", [](nyx_hip_lambert_grid_query_t &c) { c.n_arr = 2147483648LL; }, "n_arr = 2147483648"},
        {"has_tof 2", [](nyx_hip_lambert_grid_query_t &c) { c.has_tof = 2; }, "has_tof = 2, 0 or 1"},
        {"dep step", [](nyx_hip_lambert_grid_query_t &c) { c.dep_step_ns = 0; }, "dep_step_ns must be > 0"},
        {"arr step", [](nyx_hip_lambert_grid_query_t &c) { c.arr_step_ns = -3; }, "arr_step_ns must be > 0"},
        {"arr step unread", [](nyx_hip_lambert_grid_query_t &c) { c.arr_step_ns = 0; c.has_tof = 1; }, ""},
        {"tof step", [](nyx_hip_lambert_grid_query_t &c) { c.tof_step_ns = 0; c.has_tof = 1; }, "tof_step_ns must be > 0"},
        {"tof step unread", [](nyx_hip_lambert_grid_query_t &c) { c.tof_step_ns = 0; }, ""},
        {"chain 5", [](nyx_hip_lambert_grid_query_t &c) { c.arr.n_chain = 5; }, "arr.n_chain = 5, 0 .. 4 segments"},
        {"chain -1", [](nyx_hip_lambert_grid_query_t &c) { c.dep.n_chain = -1; }, "dep.n_chain = -1"},
        {"segment -1", [](nyx_hip_lambert_grid_query_t &c) { c.centre.chain_segment[1] = -1; }, "centre.chain_segment[1] = -1 is not a segment of the context"},
        {"sign 0", [](nyx_hip_lambert_grid_query_t &c) { c.arr.chain_sign[2] = 0; }, "arr.chain_sign[2] = 0, +1 or -1"},
        {"sign beyond the chain", [](nyx_hip_lambert_grid_query_t &c) { c.arr.chain_sign[3] = 7; }, ""},
        {"dep is the centre", [](nyx_hip_lambert_grid_query_t &c) { c.dep = c.centre; }, "the departure body's chain is the centre's"},
        {"arr is the centre", [](nyx_hip_lambert_grid_query_t &c) { c.arr = c.centre; }, "the arrival body's chain is the centre's"},
        {"both empty", [](nyx_hip_lambert_grid_query_t &c) { c.centre.n_chain = 0; }, "the departure body's chain is the centre's"},
        {"same body both ends", [](nyx_hip_lambert_grid_query_t &c) { c.dep = c.arr; }, ""},
        {"segment beyond the context", [](nyx_hip_lambert_grid_query_t &c) { c.arr.chain_segment[0] = 5; }, "arr.chain_segment[0] = 5 is not a segment of the context (0 .. 4)"},
        {"order: sizes before chains", [](nyx_hip_lambert_grid_query_t &c) { c.n_dep = -1; c.arr.n_chain = 9; }, "n_dep = -1"},
        {"order: query before context", [](nyx_hip_lambert_grid_query_t &c) { c.arr.chain_segment[0] = 5; c.dep = c.centre; }, "the departure body's chain"},
    };
    for (auto &c : grid) {
        nyx_hip_lambert_grid_query_t e = good_grid();
        c.edit(e);
        expect(c.label, grid_checks(ctx, &e, x, st), c.why);
    }
    expect("grid: values", grid_checks(ctx, &g, nullptr, st), "values and status arrays required");
    expect("grid: status", grid_checks(ctx, &g, x, nullptr), "values and status arrays required");
    expect("grid: swap", grid_checks(ctx, &g, x, st, true), "integration-frame swap", NYX_HIP_RC_UNSUPPORTED);
    nyx_hip_lambert_grid_query_t e = good_grid();
    e.arr.chain_segment[0] = 5;
    expect("grid: segments before the swap", grid_checks(ctx, &e, x, st, true), "not a segment of the context", NYX_HIP_RC_BAD_ARG);
    // the chain as the kernel walks it
    DevSeg ctx_seg[kSeg];
    std::memset(ctx_seg, 0, sizeof ctx_seg);
    for (int i = 0; i < kSeg; ++i) ctx_seg[i].offset = 100 * i;
    const ResolvedChain ch = resolve_chain(chain_view(g.arr), ctx_seg);
    CHECK(ch.n_chain == 3 && ch.seg[0].offset == 400 && ch.seg[1].offset == 100 && ch.seg[2].offset == 0 && ch.sign[0] == 1.0 && ch.sign[1] == -1.0 && ch.sign[3] == 0.0,
          "resolve_chain");
}

// ---- the device blocks of the two host flavours against what abi.cpp computed inline before the header had them, restated here
// (block_check.h)
static void check_block() {
    for (int64_t n : {0, 1, 63, 65})
        for (int P : {1, 8}) {
            const size_t row = (size_t)n * sizeof(double), in = 13 * row, vals = (size_t)P * row;   // nyx_hip_lambert_batch
            check_parts(lambert_batch_block(n, P), {0, 6 * row, 12 * row, in, in + vals}, {6 * row, 6 * row, row, vals, (size_t)n * sizeof(int32_t)},
                        in + vals + (size_t)n * sizeof(int32_t), LBB_STATUS, "batch", (long long)n, P, 0);
        }
    const int64_t grids[][2] = {{0, 0}, {0, 5}, {1, 1}, {7, 9}, {13, 5}};   // 0, 0, 1, 63 and 65 cells
    for (const auto &g : grids)
        for (int P : {1, 8}) {
            const size_t cells = (size_t)g[0] * (size_t)g[1], vals = (size_t)P * cells * sizeof(double);   // nyx_hip_lambert_grid
            check_parts(lambert_grid_block(g[0], g[1], P), {0, vals}, {vals, cells * sizeof(int32_t)}, vals + cells * sizeof(int32_t), LGB_STATUS, "grid",
                        (long long)cells, P, 0);
        }
}

struct Seg { double init, interval; int n_rec, n_coef; std::vector<double> rec; };
struct Prob { nyx_hip_lambert_query_t q; double mu, rv1[6], rv2[6], tof; };
struct Cell { double et_dep, et_arr, tof, mu; };

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

static void print_solution(int st, const LmbSol &s) {
    for (int p = 0; p < NYX_HIP_LMB_COUNT; ++p) std::printf(" %a", st == NYX_HIP_LMB_OK ? lmb_param(p, s) : (double)NAN);
    std::printf("\n");
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
    nyx_hip_lambert_chain_t chains[3];   // departure, arrival, centre
    std::memset(chains, 0, sizeof chains);
    for (nyx_hip_lambert_chain_t &c : chains) {
        c.n_chain = (int)ri(f);
        if (c.n_chain < 0 || c.n_chain > NYX_HIP_MAX_CHAIN) { std::printf("FAIL: n_chain\n"); std::exit(2); }
        for (int k = 0; k < c.n_chain; ++k) {
            c.chain_segment[k] = (int)ri(f); c.chain_sign[k] = (int)ri(f);
            if (c.chain_segment[k] < 0 || c.chain_segment[k] >= n_seg) { std::printf("FAIL: chain segment\n"); std::exit(2); }
        }
    }
    const int n_prob = (int)ri(f);
    if (n_prob < 0 || n_prob > 100000) { std::printf("FAIL: n_prob\n"); std::exit(2); }
    std::vector<Prob> probs((size_t)n_prob);
    for (Prob &p : probs) {
        p.q = good_solver();
        p.q.way = (int)ri(f); p.q.n_revs = (int)ri(f); p.q.high_path = (int)ri(f); p.q.max_iter = (int)ri(f);
        p.q.tol = rd(f); p.mu = rd(f);
        for (double &v : p.rv1) v = rd(f);
        for (double &v : p.rv2) v = rd(f);
        p.tof = rd(f);
    }
    const int n_cell = (int)ri(f);
    if (n_cell < 0 || n_cell > 100000) { std::printf("FAIL: n_cell\n"); std::exit(2); }
    std::vector<Cell> cells((size_t)n_cell);
    for (Cell &c : cells) { c.et_dep = rd(f); c.et_arr = rd(f); c.tof = rd(f); c.mu = rd(f); }
    std::fclose(f);

    for (int c = 0; c < n_prob; ++c) {
        LmbSol s;
        std::memset(&s, 0, sizeof s);
        const int st = lmb_solve(probs[c].rv1, probs[c].rv2, probs[c].tof, probs[c].mu, probs[c].q, s);
        std::printf("sol %d %d", c, st);
        print_solution(st, s);
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
                    for (int k = 0; k < 3; ++k)
                        for (int j = 0; j < 16; ++j) records.push_back(j < s.n_coef ? src[2 + k * s.n_coef + j] : 0.0);
                }
            } else {
                d.stride = src_stride;
                records.insert(records.end(), s.rec.begin(), s.rec.end());
            }
        }
        const ResolvedChain dep = resolve_chain(chain_view(chains[0]), ctx_seg), arr = resolve_chain(chain_view(chains[1]), ctx_seg),
                            centre = resolve_chain(chain_view(chains[2]), ctx_seg);
        const nyx_hip_lambert_query_t q = good_solver();
        for (int c = 0; c < n_cell; ++c) {
            // a cell of the grid kernel, step by step: the two body states about the centre, then the solve
            double rv1[6], rv2[6];
            const int st1 = lmb_body_state(dep, centre, records.data(), cells[c].et_dep, rv1);
            const int st2 = lmb_body_state(arr, centre, records.data(), cells[c].et_arr, rv2);
            LmbSol s;
            std::memset(&s, 0, sizeof s);
            const int st = st1 != NYX_HIP_OK || st2 != NYX_HIP_OK ? NYX_HIP_LMB_EPHEM_RANGE : lmb_solve(rv1, rv2, cells[c].tof, cells[c].mu, q, s);
            std::printf("cell %d %d %d", layout, c, st1);
            for (double v : rv1) std::printf(" %a", v);
            std::printf(" %d", st2);
            for (double v : rv2) std::printf(" %a", v);
            std::printf(" %d", st);
            print_solution(st, s);
        }
    }
    // one core, the problems over and over: the CPU baseline of tools/time_lambert.py's figures
    if (n_prob > 0) {
        const int rounds = 50;
        double sink = 0.0;
        const auto t0 = std::chrono::steady_clock::now();
        for (int r = 0; r < rounds; ++r)
            for (const Prob &p : probs) {
                LmbSol s;
                if (lmb_solve(p.rv1, p.rv2, p.tof, p.mu, p.q, s) == NYX_HIP_LMB_OK) sink += s.x;
            }
        const double ns = std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count();
        std::printf("time %.1f %d %a\n", ns / (rounds * (double)n_prob), rounds * n_prob, sink);
    }
}

int main(int argc, char **argv) {
    refusals();
    check_block();
    if (argc > 1) evaluate(argv[1]);
    if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
    std::printf("ok\n");
    return 0;
}
