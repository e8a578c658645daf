// Stand-alone check of the host side of the entries that run the propagator (nyx_amd/csrc/run_host.h and the predicates beside
// pick_quad in launch_plan.h) - g++ only, no HIP, no GPU (tests/test_run_host.py).
//   run_host_check REFUSALS_OUT
// writes the refusal cases (run_host_cases.h) to REFUSALS_OUT, one line per case (compared with tests/golden/run_check.txt by the
// test); checks the device blocks of predict_until, until_event and ensemble_moments, the segments of a covariance-mapping loop and
// the three launch predicates against what abi.cpp computed inline before the header existed, restated here.  "ok" last.
#include <cstdint>
#include <cstdio>
#include <map>
#include <memory>
#include <vector>

#include "run_host_cases.h"

#include "../../nyx_amd/csrc/launch_plan.h"
#include "../../nyx_amd/csrc/run_host.h"

static int g_fail = 0;
#define CHECK(cond, ...)                                                              \
    do {                                                                              \
        if (!(cond)) {                                                                \
            if (++g_fail <= 30) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                             \
    } while (0)

// an entry's checks in the order abi.cpp runs them: its own, then the bracket's
struct Header {
    static Outcome of(const Refusal &r) { return {r.rc, r.msg}; }
    static Outcome then_run(const Refusal &first, nyx_hip_ctx *ctx, const nyx_hip_states_t *in, const nyx_hip_states_t *out, bool stm) {
        return first ? of(first) : of(check_run(ctx, in, out, stm));
    }
    static Outcome states(const nyx_hip_states_t *s, const char *what) { return of(check_states(s, what)); }
    static Outcome run(nyx_hip_ctx *ctx, const nyx_hip_states_t *in, const nyx_hip_states_t *out, bool stm) { return of(check_run(ctx, in, out, stm)); }
    static Outcome with_traj(nyx_hip_ctx *ctx, const nyx_hip_states_t *in, const nyx_hip_states_t *out, const nyx_hip_traj_t *traj, bool stm) {
        return then_run(check_traj_wanted(traj), ctx, in, out, stm);
    }
    static Outcome sharded(nyx_hip_ctx *const *ctxs, int32_t n_ctx, const nyx_hip_states_t *in, const nyx_hip_states_t *out, const nyx_hip_traj_t *traj) {
        return of(check_sharded(ctxs, n_ctx, in, out, traj));
    }
    static Outcome event(nyx_hip_ctx *ctx, const nyx_hip_states_t *in, const nyx_hip_event_t *e, const nyx_hip_states_t *out, const nyx_hip_traj_t *traj, bool stm) {
        return then_run(check_event(ctx, e, traj), ctx, in, out, stm);
    }
    static Outcome predict(nyx_hip_ctx *ctx, uint32_t flags, const nyx_hip_states_t *in, const nyx_hip_predict_t *cfg, nyx_hip_estimates_t *est,
                           const nyx_hip_states_t *out, const nyx_hip_predict_history_t *hist) {
        return then_run(check_predict(ctx, flags, cfg, est, hist), ctx, in, out, false);
    }
    static Outcome moments_device(nyx_hip_ctx *ctx, const nyx_hip_states_t *s, double *out55) { return of(check_moments(ctx, s, out55, false)); }
    static Outcome moments_host(nyx_hip_ctx *ctx, const nyx_hip_states_t *s, double *out55) { return of(check_moments(ctx, s, out55, true)); }
    static Outcome eval_host(nyx_hip_ctx *ctx, const nyx_hip_traj_t *traj, int64_t n, const int64_t *query, int64_t m, int64_t step_ns,
                             const nyx_hip_traj_t *out, int32_t *status, int mode) {
        return of(check_traj_eval_host(ctx, traj, n, query, m, step_ns, out, status, mode));
    }
};

// parts in the order of their enum, each starting where the one before ends; total = their sum
template <int N> static void check_parts(const Block<N> &b, const char *what, long long n) {
    size_t at = 0;
    for (int k = 0; k < N; ++k) {
        CHECK(b[k].at == at, "%s n=%lld: part %d at %zu, the parts before it end at %zu", what, n, k, b[k].at, at);
        at += b[k].bytes;
    }
    CHECK(b.total == at, "%s n=%lld: total %zu, parts %zu", what, n, b.total, at);
}

// ---- the block of predict_until against the eight-plus-five allocations it replaces: covar n*81*8, sdev n*9*8, work n*(6*8 + 2*4),
// and for every history array asked for, with capacity * n > 0 slots, slots * width * 8
static void check_predict_block() {
    const size_t width[5] = {1, 9, 81, 81, 9};
    alignas(8) static char fake[8];
    char *const base = fake;  // (only offsets from it are formed, nothing is read)
    for (int64_t n : {0, 1, 2, 15, 16, 17, 63, 65})
        for (int64_t capacity : {0, 1, 3})
            for (int subset = 0; subset < 32; ++subset)
                {
                    nyx_hip_predict_history_t h = {capacity, subset & 1 ? i64 : nullptr, subset & 2 ? f64 : nullptr, subset & 4 ? f64 : nullptr,
                                                   subset & 8 ? f64 : nullptr, subset & 16 ? f64 : nullptr, i32};
                    const Block<P_COUNT> b = predict_block(n, h);
                    const long long c[3] = {(long long)n, (long long)capacity, subset};
#define AT "n=%lld capacity=%lld subset=%lld", c[0], c[1], c[2]
                    check_parts(b, "predict", n);
                    const size_t slots = (size_t)capacity * (size_t)n;
                    size_t parent = (size_t)n * 81 * 8 + (size_t)n * 9 * 8 + (size_t)n * (6 * 8 + 2 * 4);
                    for (int k = 0; k < 5; ++k) {
                        const size_t want = (subset >> k & 1) ? slots * width[k] * 8 : 0;
                        CHECK(b[P_H_EPOCH + k].bytes == want, AT);
                        parent += want;
                    }
                    CHECK(b.total == parent, AT);  // (no padding: every part before the int32 rows is a multiple of 8 bytes)
                    CHECK(b[P_COVAR].bytes == (size_t)n * 81 * 8 && b[P_SDEV].bytes == (size_t)n * 9 * 8, AT);
                    for (int k = P_PREV_EPOCH; k <= P_INIT_EPOCH; ++k) CHECK(b[k].bytes == (size_t)n * 8, AT);
                    CHECK(b[P_STATUS].bytes == (size_t)n * 4 && b[P_N_UPDATES].bytes == (size_t)n * 4, AT);
                    for (int k = 0; k < P_STATUS; ++k) CHECK(b[k].at % 8 == 0 && b[k].bytes % 8 == 0, AT);   // doubles and int64
                    CHECK(b[P_STATUS].at % 4 == 0 && b[P_N_UPDATES].at % 4 == 0 && P_N_UPDATES == P_COUNT - 1 && P_STATUS == P_COUNT - 2, AT);
                    // the history is contiguous, the deviations in front of it and status behind: what the entry clears is one piece
                    // from b[P_H_EPOCH].at (b[P_SDEV].at for a caller without deviations) to b[P_STATUS].at
                    CHECK(b[P_H_SDEV].at + b[P_H_SDEV].bytes == b[P_STATUS].at && b[P_SDEV].at + b[P_SDEV].bytes == b[P_H_EPOCH].at, AT);
                    for (int k = P_H_EPOCH; k < P_H_SDEV; ++k) CHECK(b[k].at + b[k].bytes == b[k + 1].at, AT);
                    // bind_predict: every pointer at its part, an absent part null
                    PredictArgs a;
                    std::memset(&a, 0, sizeof a);
                    bind_predict(a, base, b);
                    const void *got[P_COUNT] = {a.covar, a.prev_epoch, a.dur, a.acc_n_acc, a.acc_n_rej, a.acc_n_evals, a.init_epoch, a.state_dev,
                                                a.hist.epoch_ns, a.hist.state, a.hist.stm, a.hist.covar, a.hist.state_dev, a.status, a.hist.n_updates};
                    for (int k = 0; k < P_COUNT; ++k) {
                        CHECK(got[k] == (b[k].bytes ? base + b[k].at : nullptr), AT);
                        for (int j = 0; j < k; ++j)  // no two parts alias: [at, at + bytes) are disjoint
                            CHECK(!b[k].bytes || !b[j].bytes || b[j].at + b[j].bytes <= b[k].at, AT);
                    }
                    for (int k = 0; k < 5; ++k) CHECK((got[P_H_EPOCH + k] != nullptr) == ((subset >> k & 1) && slots > 0), AT);
                    CHECK(a.n == 0 && a.stm == nullptr && a.hist.capacity == 0, AT);  // (bind_predict sets pointers of the block only)
#undef AT
                }
}

// ---- until_event: n * 16 bytes, prev (f64) / count / found (i32); ensemble_moments: nine rows of n doubles and the status words
// (the parent allocated max(n, 1) per row and always room for the status: the block differs by that padding alone)
static void check_small_blocks() {
    for (int64_t n : {0, 1, 2, 15, 16, 17, 63, 65}) {
        const auto e = event_block(n);
        check_parts(e, "event", n);
        CHECK(e.total == (size_t)n * 16 && e[E_PREV].bytes == (size_t)n * 8 && e[E_COUNT].bytes == (size_t)n * 4 && e[E_FOUND].bytes == (size_t)n * 4, "n=%lld", (long long)n);
        CHECK(e[E_PREV].at == 0 && e[E_COUNT].at == (size_t)n * 8 && e[E_FOUND].at == (size_t)n * 12, "n=%lld", (long long)n);
        for (int status = 0; status < 2; ++status) {
            const auto m = moments_block(n, status != 0);
            check_parts(m, "moments", n);
            const size_t n1 = n > 0 ? (size_t)n : 1, parent = 9 * n1 * 8 + n1 * 4;
            for (int k = 0; k < 9; ++k) CHECK(m[k].at == (size_t)k * (size_t)n * 8 && m[k].bytes == (size_t)n * 8, "n=%lld row %d", (long long)n, k);
            CHECK(m[M_STATUS].bytes == (status ? (size_t)n * 4 : 0) && m[M_STATUS].at % 8 == 0, "n=%lld", (long long)n);
            CHECK(parent - m.total == (status && n > 0 ? 0 : n1 * 4) + (n > 0 ? 0 : 9 * 8), "n=%lld: %zu, the parent %zu", (long long)n, m.total, parent);
        }
    }
}

// ---- predict_segments against the loop of nyx_hip_predict_until
static void check_segments() {
    auto parent = [](const std::vector<int64_t> &epochs, int64_t end_epoch_ns, int64_t max_step_ns) {
        int64_t n_seg = 1;
        for (size_t i = 0; i < epochs.size(); ++i) {
            const int64_t span = end_epoch_ns - epochs[i];
            if (span > 0) n_seg = std::max(n_seg, (span + max_step_ns - 1) / max_step_ns);
        }
        return n_seg;
    };
    auto one = [&](const std::vector<int64_t> &epochs, int64_t end, int64_t step, int64_t want = -1) {
        const int64_t got = predict_segments(epochs.data(), (int64_t)epochs.size(), end, step);
        CHECK(got == parent(epochs, end, step), "end %lld step %lld: %lld segments, the loop had %lld", (long long)end, (long long)step, (long long)got,
              (long long)parent(epochs, end, step));
        CHECK(want < 0 || got == want, "end %lld step %lld: %lld segments, not %lld", (long long)end, (long long)step, (long long)got, (long long)want);
    };
    one({}, 100, 7, 1);                        // no trajectory
    one({100}, 100, 7, 1);                     // span 0
    one({101, 500}, 100, 7, 1);                // spans < 0: every trajectory already finished
    one({0}, 1, 7, 1);
    for (int64_t step : {1, 7, 60, 1000000007})
        for (int64_t k : {1, 2, 3, 1000}) {    // a span of exactly k steps, and 1 ns around it
            one({0}, k * step, step, k);
            one({0}, k * step + 1, step, k + 1);
            one({5}, 5 + k * step - 1, step, step == 1 && k == 1 ? 1 : (step == 1 ? k - 1 : k));
        }
    one({0, 30, 59, 60, 61, 1000}, 600, 60, 10);   // ragged starts: the longest decides, the finished ones count nothing
    one({590, 0, 700}, 600, 60, 10);
    one({-600}, 600, 60, 20);
    const int64_t half = INT64_MAX / 2;
    one({0}, half, 1000000000, (half + 999999999) / 1000000000);   // a span near INT64_MAX / 2
    one({0, 5}, half - 1, half, 1);
    one({0, 5}, half - 1, half - 1000, 2);
}

// ---- the three launch predicates, over a grid on both sides of every threshold, against the expressions of launch_here and
// nyx_hip_predict_until
static void check_predicates() {
    nyx_hip_tuning_t tune = NYX_HIP_TUNING_DEFAULT;
    std::vector<int32_t> col_len;
    const double rh[3] = {0.0, 0.0, 0.0};
    WeightMap weights;
    const std::unique_ptr<DevCfg> dc(new DevCfg);
    std::memset(dc.get(), 0, sizeof(DevCfg));
    dc->init_step_ns = 60;
    const WKey key(8, 1, 1, -1), other(16, 1, 1, -1);
    for (int sched : {NYX_HIP_SCHED_MODEL, NYX_HIP_SCHED_CALIBRATED, NYX_HIP_SCHED_EXPLICIT})
        for (int grav = 0; grav < 2; ++grav)
            for (int nw : {7, 8, 16})
                for (int64_t n : {15, 16, 17, 63, 64, 65})
                    for (int known = 0; known < 3; ++known)   // no weights, this shape's, another shape's
                        for (int plain = 0; plain < 2; ++plain)
                            for (int64_t span : {(int64_t)99 * 60, (int64_t)100 * 60 - 1, (int64_t)100 * 60, INT64_MAX}) {
                                tune.schedule = sched;
                                dc->has_grav = grav;
                                weights.clear();
                                if (known) weights[known == 1 ? key : other] = {};
                                const PlanInputs in{tune, col_len, rh, 0, 0, 256, 0, -1, weights};
                                const bool on = sched == NYX_HIP_SCHED_CALIBRATED;
                                const bool want_launch = plain && on && grav && nw >= 8 && n >= 64 && span >= 100 * dc->init_step_ns && !weights.count(key);
                                const bool want_predict = on && grav && nw >= 8 && n >= 16 && !weights.count(key);
                                CHECK(calibrates_first(in, *dc, key, nw, n, 64, plain != 0, span, 100) == want_launch,
                                      "sched %d grav %d waves %d n %lld known %d plain %d span %lld", sched, grav, nw, (long long)n, known, plain, (long long)span);
                                CHECK(calibrates_first(in, *dc, key, nw, n, 16, true, 0, 0) == want_predict, "sched %d grav %d waves %d n %lld known %d", sched, grav,
                                      nw, (long long)n, known);
                            }
    // the fused loop: no swap, the switch clear, the quad layout (pick_quad: by flags, forced layout, tuning, ensemble size)
    for (int swap : {0, 1, 3})
        for (int flag : {0, 0x20000000, 0x20000400, 0x400})
            for (uint32_t flags : {0u, (uint32_t)NYX_HIP_FLAG_STM, (uint32_t)(NYX_HIP_FLAG_STM | NYX_HIP_FLAG_STM_TEXTBOOK)})
                for (int forced : {-1, 0, 1})
                    for (int det = 0; det < 2; ++det)
                        for (int64_t n : {1, 16, 17, 32 * 256, 32 * 256 + 1}) {
                            tune = NYX_HIP_TUNING_DEFAULT;
                            tune.debug_flags = flag;
                            tune.deterministic = det;
                            dc->flags = flags;
                            weights.clear();
                            const PlanInputs in{tune, col_len, rh, 0, 0, 256, 0, forced, weights};
                            const bool want = swap == 0 && !(flag & 0x20000000) && pick_quad(in, *dc, n);
                            CHECK(predict_fused(in, *dc, n, swap) == want, "swap %d flag %#x flags %u forced %d det %d n %lld", swap, flag, flags, forced, det, (long long)n);
                            // (pick_quad itself, at its threshold of two quad workgroups per CU: launch_plan_check.cpp)
                            if (swap == 0 && flag == 0 && flags == NYX_HIP_FLAG_STM && forced < 0 && !det && tune.stm_quad < 0)
                                CHECK(predict_fused(in, *dc, n, 0) == (n <= 32 * 256), "n %lld", (long long)n);
                        }
}

int main(int argc, char **argv) {
    if (argc < 2) { std::printf("usage: run_host_check REFUSALS_OUT\n"); return 2; }
    std::FILE *f = std::fopen(argv[1], "w");
    if (!f) { std::printf("cannot write %s\n", argv[1]); return 2; }
    run_refusal_cases<Header>(f);
    std::fclose(f);
    check_predict_block();
    check_small_blocks();
    check_segments();
    check_predicates();
    if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
    std::printf("ok\n");
    return 0;
}
