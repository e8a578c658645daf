// target_host_check.cpp — the host side of the targeter, stand-alone (its own main; g++ only, no HIP, no GPU):
// nyx_amd/csrc/target_args.h (what the two entries refuse, as abi.cpp chains the checks) and THE KERNELS' OWN per-run code compiled for
// the host, nyx_amd/csrc/target_dev.h (the seed, the start states of a round, the step, the corrected state).  Run by
// tests/test_target_host_cxx.py, plain and under the address and undefined-behaviour sanitizers.
//
// Without an argument: the refusal table, "ok" last.  With an input file (hex floats): cases
//   V O ITERATIONS FRAME / V x (component perturbation guess max_step max_value min_value) / O x (param desired tol mult add) / MU
//   xi_start[6] / ROUNDS / per round (1 + V) x (status y[6]): the final states of the round, about the objective target
// and for every case the loop of nyx_hip_target_batch_device on them (%a):
//   "seed CASE total[V]", "start CASE ROUND K x[6]" for the 1 + V start states of every round that is run,
//   "step CASE ROUND status err[O] total[V]" per round (status -1: the run goes on), "corrected CASE x[6]" when the run ends.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../nyx_amd/csrc/target_dev.h"

static int g_fail = 0;
#define CHECK(cond, ...)                                                              \
    do {                                                                              \
        if (!(cond)) {                                                                \
            if (++g_fail <= 30) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                             \
    } while (0)

#include "block_check.h"

static nyx_hip_target_query_t good_query() {
    nyx_hip_target_query_t q;
    std::memset(&q, 0, sizeof q);
    q.n_vars = 3; q.n_objs = 2; q.iterations = 100; q.correction_frame = NYX_HIP_FRAME_INERTIAL;
    for (int j = 0; j < 3; ++j) {
        q.var_component[j] = NYX_HIP_VARY_VELOCITY_X + j; q.var_perturbation[j] = 1e-4; q.var_max_step[j] = 0.2; q.var_max_value[j] = 5.0; q.var_min_value[j] = -5.0;
    }
    q.obj_param[0] = NYX_HIP_SP_ECCENTRICITY; q.obj_desired[0] = 0.4; q.obj_tolerance[0] = 1e-5; q.obj_mult[0] = 1.0;
    q.obj_param[1] = NYX_HIP_SP_SEMI_MAJOR_AXIS; q.obj_desired[1] = 8100.0; q.obj_tolerance[1] = 0.1; q.obj_mult[1] = 1.0;
    q.n_chain = 2; q.chain_segment[0] = 3; q.chain_sign[0] = 1; q.chain_segment[1] = 2; q.chain_sign[1] = -1;
    q.mu_km3_s2 = 398600.4;
    return q;
}

struct Io {   // a batch and a result whose arrays exist (never read or written by a check)
    int64_t e[2];
    double d[2];
    int32_t s[2];
    nyx_hip_states_t in;
    nyx_hip_target_result_t res;
    Io() {
        std::memset(&in, 0, sizeof in);
        std::memset(&res, 0, sizeof res);
        fill(in);
        fill(res.corrected);
        fill(res.achieved);
        in.n = 2;
        res.status = s; res.iterations = s; res.correction = d; res.achieved_errors = d;
    }
    void fill(nyx_hip_states_t &v) { v.epoch_ns = e; v.x_km = v.y_km = v.z_km = v.vx_km_s = v.vy_km_s = v.vz_km_s = d; }
};

static void refused(const char *label, const Refusal &r, int rc, const char *why) {
    CHECK(r.rc == rc && std::strstr(r.msg, why) != nullptr, "%s: rc %d, \"%s\" (wanted %d, \"%s\")", label, r.rc, r.msg, rc, why);
}

static void refusal_table() {
    const nyx_hip_ctx *ctx = (const nyx_hip_ctx *)(uintptr_t)1;   // never dereferenced by check_target
    Io io;
    nyx_hip_target_query_t q = good_query();
    CHECK(!check_target(ctx, &io.in, &q, &io.res), "the good query is accepted");
    CHECK(!check_target_context(q, 4, false, false), "and so by a context of four segments");
    refused("ctx", check_target(nullptr, &io.in, &q, &io.res), NYX_HIP_RC_BAD_ARG, "null ctx");
    refused("query", check_target(ctx, &io.in, nullptr, &io.res), NYX_HIP_RC_BAD_ARG, "target_batch: null query");
    refused("result", check_target(ctx, &io.in, &q, nullptr), NYX_HIP_RC_BAD_ARG, "target_batch: null result");
#define WITH(stmt, rc, why) do { nyx_hip_target_query_t t = good_query(); stmt; refused(#stmt, check_target(ctx, &io.in, &t, &io.res), rc, why); } while (0)
    WITH(t.n_vars = 0, NYX_HIP_RC_BAD_ARG, "n_vars = 0, 1 .. 6 variables");
    WITH(t.n_vars = 7, NYX_HIP_RC_BAD_ARG, "n_vars = 7");
    WITH(t.n_objs = 7, NYX_HIP_RC_BAD_ARG, "n_objs = 7, 1 .. 6 objectives");
    WITH(t.iterations = 1001, NYX_HIP_RC_BAD_ARG, "iterations = 1001, 0 .. 1000");
    WITH(t.iterations = -1, NYX_HIP_RC_BAD_ARG, "iterations = -1");
    WITH(t.correction_frame = NYX_HIP_FRAME_RIC, NYX_HIP_RC_BAD_ARG, "correction_frame = 1, inertial (0) or VNC (2)");
    WITH(t.var_component[2] = 6, NYX_HIP_RC_BAD_ARG, "var_component[2] = 6 is not a nyx_hip_target_vary");
    WITH(t.var_perturbation[1] = 0.0, NYX_HIP_RC_BAD_ARG, "var_perturbation[1] must be finite and not zero");
    WITH(t.var_perturbation[1] = NAN, NYX_HIP_RC_BAD_ARG, "var_perturbation[1]");
    WITH(t.var_init_guess[0] = INFINITY, NYX_HIP_RC_BAD_ARG, "var_init_guess[0] must be finite");
    WITH(t.var_max_step[0] = -1.0, NYX_HIP_RC_BAD_ARG, "var_max_step[0] must be >= 0");
    WITH(t.var_max_value[0] = -1.0, NYX_HIP_RC_BAD_ARG, "var_max_value[0] must be >= 0");
    WITH(t.var_min_value[1] = 5.5, NYX_HIP_RC_BAD_ARG, "var_min_value[1] must be <= var_max_value[1]");
    WITH((t.correction_frame = NYX_HIP_FRAME_VNC, t.var_component[1] = NYX_HIP_VARY_POSITION_Z), NYX_HIP_RC_BAD_ARG, "var_component[1] is a position");
    WITH(t.obj_param[1] = NYX_HIP_FRM_COUNT, NYX_HIP_RC_BAD_ARG, "obj_param[1] = 25 is not a nyx_hip_frame_param");
    WITH(t.obj_tolerance[0] = -1.0, NYX_HIP_RC_BAD_ARG, "obj_tolerance[0] must be finite and >= 0");
    WITH(t.obj_tolerance[0] = NAN, NYX_HIP_RC_BAD_ARG, "obj_tolerance[0]");
    WITH(t.n_chain = 5, NYX_HIP_RC_BAD_ARG, "n_chain = 5, 0 .. 4 segments");
    WITH(t.chain_segment[0] = -1, NYX_HIP_RC_BAD_ARG, "chain_segment[0] = -1 is not a segment of the context");
    WITH(t.chain_sign[1] = 2, NYX_HIP_RC_BAD_ARG, "chain_sign[1] = 2, +1 or -1");
    WITH(t.mu_km3_s2 = 0.0, NYX_HIP_RC_BAD_ARG, "mu_km3_s2 must be finite and > 0");
    // which check wins: the first of the header's list
    WITH((t.n_vars = 0, t.n_objs = 0, t.mu_km3_s2 = 0.0), NYX_HIP_RC_BAD_ARG, "n_vars = 0");
    WITH((t.iterations = -5, t.correction_frame = 9, t.var_component[0] = 9), NYX_HIP_RC_BAD_ARG, "iterations = -5");
    WITH((t.var_max_step[0] = -1.0, t.var_component[1] = 9), NYX_HIP_RC_BAD_ARG, "var_max_step[0]");
    WITH((t.var_component[2] = 9, t.obj_param[0] = 99), NYX_HIP_RC_BAD_ARG, "var_component[2] = 9");
    WITH((t.obj_param[0] = 99, t.n_chain = 7), NYX_HIP_RC_BAD_ARG, "obj_param[0] = 99");
#undef WITH
    {   // the batch, the outputs, the hyperdual request: behind the query, in this order
        Io bad;
        bad.in.vz_km_s = nullptr;
        nyx_hip_target_query_t t = good_query();
        refused("in", check_target(ctx, &bad.in, &t, &bad.res), NYX_HIP_RC_BAD_ARG, "in: epoch and the six Cartesian arrays are mandatory");
        t.mu_km3_s2 = -1.0;
        refused("mu before in", check_target(ctx, &bad.in, &t, &bad.res), NYX_HIP_RC_BAD_ARG, "mu_km3_s2");
        Io out;
        out.res.correction = nullptr;
        t = good_query();
        refused("outputs", check_target(ctx, &out.in, &t, &out.res), NYX_HIP_RC_BAD_ARG, "status, iterations, correction and achieved_errors arrays required");
        Io st;
        st.res.achieved.epoch_ns = nullptr;
        refused("states", check_target(ctx, &st.in, &t, &st.res), NYX_HIP_RC_BAD_ARG, "corrected and achieved: epoch and the six Cartesian arrays are mandatory");
        Io dual;
        dual.in.stm = dual.d;
        refused("stm", check_target(ctx, &dual.in, &t, &dual.res), NYX_HIP_RC_UNSUPPORTED, "in->stm is given: the hyperdual targeter");
        dual.res.status = nullptr;
        refused("outputs before stm", check_target(ctx, &dual.in, &t, &dual.res), NYX_HIP_RC_BAD_ARG, "arrays required");
    }
    refused("segment", check_target_context(q, 3, false, false), NYX_HIP_RC_BAD_ARG, "chain_segment[0] = 3 is not a segment of the context (0 .. 2)");
    refused("stm context", check_target_context(q, 4, true, false), NYX_HIP_RC_UNSUPPORTED, "the context carries STMs");
    refused("swap", check_target_context(q, 4, false, true), NYX_HIP_RC_UNSUPPORTED, "integration-frame swap");
    refused("segment before swap", check_target_context(q, 3, true, true), NYX_HIP_RC_BAD_ARG, "is not a segment of the context");
    CHECK(tgt_needs(q) == (frm_param_needs(NYX_HIP_SP_ECCENTRICITY) | frm_param_needs(NYX_HIP_SP_SEMI_MAJOR_AXIS)), "the needs of the objectives");
}

// ---- the device block of the host flavour's outputs against what nyx_hip_target_batch computed inline before the header had it,
// restated here (block_check.h), and the result bound into it against that entry's loop over the two states
static void check_block() {
    const int shapes[][2] = {{1, 1}, {3, 2}, {6, 6}};
    for (int64_t n : {0, 1, 63, 65})
        for (const auto &vo : shapes) {
            const int V = vo[0], O = vo[1];
            const size_t row = (size_t)n * sizeof(double), corr = (size_t)V * row, errs = (size_t)O * row, words = (size_t)n * sizeof(int32_t);
            const Block<TGB_PARTS> b = target_block(n, V, O);
            check_parts(b, {0, corr, corr + errs, corr + errs + 14 * row, corr + errs + 28 * row, corr + errs + 28 * row + words}, {corr, errs, 14 * row, 14 * row, words, words},
                        corr + errs + 28 * row + 2 * (size_t)n * sizeof(int32_t), TGB_STATUS, "target", (long long)n, V, O);
            std::vector<char> mem(b.total + 8);
            char *base = mem.data();
            nyx_hip_target_result_t d;
            std::memset(&d, 0, sizeof d);
            bind_target_result(d, base, b);
            CHECK(d.correction == (double *)base && d.achieved_errors == (double *)(base + corr), "target n=%lld (%d, %d): correction, errors", (long long)n, V, O);
            CHECK(d.status == (int32_t *)(base + corr + errs + 28 * row) && d.iterations == d.status + n, "target n=%lld (%d, %d): status, iterations", (long long)n, V, O);
            const nyx_hip_states_t *views[2] = {&d.corrected, &d.achieved};
            for (int s = 0; s < 2; ++s) {
                char *at = base + corr + errs + (size_t)s * 14 * row;
                CHECK(views[s]->n == n && views[s]->epoch_ns == (int64_t *)at, "target n=%lld (%d, %d) state %d: n, epochs", (long long)n, V, O, s);
                for (int k = 0; k < kStateRows; ++k) {
                    CHECK(views[s]->*kStateRow[k].s == (double *)(at + (size_t)(1 + k) * row), "target n=%lld (%d, %d) state %d: row %d", (long long)n, V, O, s, k);
                    const Part p = target_row(b, TGB_CORRECTED + s, 1 + k);
                    CHECK(p.at == (size_t)(at - base) + (size_t)(1 + k) * row && p.bytes == row, "target n=%lld (%d, %d) state %d: part of row %d", (long long)n, V, O, s, k);
                }
                CHECK(views[s]->step_ns == nullptr && views[s]->stm == nullptr, "target n=%lld (%d, %d) state %d: nothing else is bound", (long long)n, V, O, s);
            }
        }
}

static double rd(FILE *f) {
    char tok[64];
    if (std::fscanf(f, "%63s", tok) != 1) { std::printf("FAIL short input\n"); std::exit(2); }
    return std::strtod(tok, nullptr);
}
static int ri(FILE *f) {
    int v = 0;
    if (std::fscanf(f, "%d", &v) != 1) { std::printf("FAIL short input\n"); std::exit(2); }
    return v;
}

static void print_starts(const nyx_hip_target_query_t &q, int c, int round, const double xs[6], const double xi[6]) {
    for (int k = 0; k <= q.n_vars; ++k) {
        double x[6];
        tgt_start_state(q, xs, xi, k, x);
        std::printf("start %d %d %d", c, round, k);
        for (int e = 0; e < 6; ++e) std::printf(" %a", x[e]);
        std::printf("\n");
    }
}

static void run_cases(const char *path) {
    FILE *f = std::fopen(path, "r");
    if (!f) { std::printf("FAIL cannot open %s\n", path); std::exit(2); }
    const int n_cases = ri(f);
    for (int c = 0; c < n_cases; ++c) {
        nyx_hip_target_query_t q;
        std::memset(&q, 0, sizeof q);
        q.n_vars = ri(f); q.n_objs = ri(f); q.iterations = ri(f); q.correction_frame = ri(f);
        for (int j = 0; j < q.n_vars; ++j) {
            q.var_component[j] = ri(f);
            q.var_perturbation[j] = rd(f); q.var_init_guess[j] = rd(f); q.var_max_step[j] = rd(f); q.var_max_value[j] = rd(f); q.var_min_value[j] = rd(f);
        }
        for (int o = 0; o < q.n_objs; ++o) {
            q.obj_param[o] = ri(f);
            q.obj_desired[o] = rd(f); q.obj_tolerance[o] = rd(f); q.obj_mult[o] = rd(f); q.obj_add[o] = rd(f);
        }
        q.mu_km3_s2 = rd(f);
        Io io;
        CHECK(!check_target((const nyx_hip_ctx *)(uintptr_t)1, &io.in, &q, &io.res), "case %d is accepted", c);
        double xs[6];
        for (int e = 0; e < 6; ++e) xs[e] = rd(f);
        const int rounds = ri(f);
        const int32_t need = tgt_needs(q);
        TgtRun run;
        tgt_seed(q, xs, run);
        std::printf("seed %d", c);
        for (int j = 0; j < q.n_vars; ++j) std::printf(" %a", run.total[j]);
        std::printf("\n");
        print_starts(q, c, 0, xs, run.xi);
        bool ended = false;
        for (int it = 0; it < rounds; ++it) {
            std::vector<double> y((size_t)(1 + q.n_vars) * 6);
            std::vector<int> st((size_t)(1 + q.n_vars));
            for (int k = 0; k <= q.n_vars; ++k) {
                st[(size_t)k] = ri(f);
                for (int e = 0; e < 6; ++e) y[(size_t)k * 6 + (size_t)e] = rd(f);
            }
            if (ended) continue;   // (never: the definition stops with the run)
            double err[TGT_MO], park[TGT_MO * TGT_MV];
            for (double &p : park) p = -12345.0;   // stale, as the device's rows are: only what the round wrote may be read
            const int status = tgt_step(q, need, it, false, [&](int k, double out[6]) -> int {
                for (int e = 0; e < 6; ++e) out[e] = y[(size_t)k * 6 + (size_t)e];
                return st[(size_t)k];
            }, park, 1, xs, 1, run, err);
            std::printf("step %d %d %d", c, it, status);
            for (int o = 0; o < q.n_objs; ++o) std::printf(" %a", err[o]);
            for (int j = 0; j < q.n_vars; ++j) std::printf(" %a", run.total[j]);
            std::printf("\n");
            if (status == TGT_GOES_ON) {
                print_starts(q, c, it + 1, xs, run.xi);
            } else {
                ended = true;
                double x[6];
                tgt_corrected(q, xs, run.total, x);
                std::printf("corrected %d", c);
                for (int e = 0; e < 6; ++e) std::printf(" %a", x[e]);
                std::printf("\n");
            }
        }
        CHECK(ended, "case %d ended within its rounds", c);
    }
    std::fclose(f);
}

int main(int argc, char **argv) {
    if (argc > 1) run_cases(argv[1]);
    else { refusal_table(); check_block(); }
    if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
    std::printf("ok\n");
    return 0;
}
