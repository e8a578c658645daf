// Stand-alone check of the host side of the sampled-series entries (nyx_amd/csrc/series_host.h) - g++ only, no HIP, no GPU
// (tests/test_series_host.py).
//   series_host_check REFUSALS_OUT
// writes the refusal cases (series_host_cases.h) to REFUSALS_OUT, one line per case (compared with tests/golden/series_check.txt by
// the test); checks the output block of the host flavours and the chunk planning of the launchers against what abi.cpp and the
// four launchers computed before the header existed, restated here.  "ok" last.
#include <cstdint>
#include <cstdio>

#include "series_host_cases.h"

#include "../../nyx_amd/csrc/series_host.h"

static int g_fail = 0;
#define CHECK(cond, ...)                                                              \
    do {                                                                              \
        if (!(cond)) {                                                                \
            if (++g_fail <= 30) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                             \
    } while (0)

struct Header {
    static Outcome of(const Refusal &r) { return {r.rc, r.msg}; }
    static Outcome traj(const nyx_hip_traj_t *t, const char *what, bool need_epochs) { return of(check_traj(t, what, need_epochs)); }
    static Outcome eval(nyx_hip_ctx *ctx, const nyx_hip_traj_t *traj, int64_t n, const int64_t *query, int64_t m, int64_t step_ns,
                        const nyx_hip_traj_t *out, int32_t *status, int mode) {
        return of(check_traj_eval(ctx, traj, n, query, m, step_ns, out, status, mode));
    }
    static Outcome values(nyx_hip_ctx *ctx, const nyx_hip_traj_t *traj, int64_t n, const nyx_hip_values_query_t *q, int64_t capacity,
                          double *values, int32_t *len) {
        return of(check_values_series(ctx, traj, n, q, capacity, values, len));
    }
    static Outcome gt(nyx_hip_ctx *ctx, const nyx_hip_traj_t *traj, int64_t n, const nyx_hip_gt_query_t *q, int64_t capacity, double *values,
                      int32_t *len) {
        return of(check_gt_series(ctx, traj, n, q, capacity, values, len));
    }
    static Outcome ric(nyx_hip_ctx *ctx, const nyx_hip_traj_t *traj, int64_t n, const nyx_hip_traj_t *ref, int64_t n_ref,
                       const nyx_hip_ric_query_t *q, int64_t capacity, double *values, int32_t *len) {
        return of(check_ric_series(ctx, traj, n, ref, n_ref, q, capacity, values, len));
    }
};

// ---- the output block: values, [moments], [first epochs], len - in that order, not overlapping, aligned, and as large as the sum
// the host flavours allocated (vbytes + mbytes + ebytes + n * sizeof(int32_t))
static void check_block() {
    for (int64_t n : {0, 1, 63, 65})
        for (int64_t capacity : {1, 3})
            for (int64_t P : {1, 6, 8})
                for (int moments = 0; moments < 2; ++moments)
                    for (int epoch0 = 0; epoch0 < 2; ++epoch0) {
                        const Block<SB_PARTS> b = series_block(P, capacity, n, moments != 0, epoch0 != 0);
                        const size_t vbytes = (size_t)P * (size_t)capacity * (size_t)n * 8;
                        const size_t mbytes = moments ? (size_t)capacity * 28 * 8 : 0;
                        const size_t ebytes = epoch0 ? (size_t)n * 8 : 0;
                        const long long c[5] = {(long long)n, (long long)capacity, (long long)P, moments, epoch0};
#define AT "n=%lld capacity=%lld P=%lld moments=%lld epoch0=%lld", c[0], c[1], c[2], c[3], c[4]
                        CHECK(b[SB_VALUES].bytes == vbytes && b[SB_MOMENTS].bytes == mbytes && b[SB_EPOCH0].bytes == ebytes && b[SB_LEN].bytes == (size_t)n * 4, AT);
                        CHECK(b[SB_VALUES].at == 0, AT);
                        CHECK(b[SB_MOMENTS].at == b[SB_VALUES].at + b[SB_VALUES].bytes, AT);   // order, and no part overlaps the next
                        CHECK(b[SB_EPOCH0].at == b[SB_MOMENTS].at + b[SB_MOMENTS].bytes, AT);
                        CHECK(b[SB_LEN].at == b[SB_EPOCH0].at + b[SB_EPOCH0].bytes, AT);
                        CHECK(b.total == b[SB_LEN].at + b[SB_LEN].bytes, AT);
                        CHECK(b.total == vbytes + mbytes + ebytes + (size_t)n * sizeof(int32_t), AT);
                        CHECK(b[SB_VALUES].at % 8 == 0 && b[SB_MOMENTS].at % 8 == 0 && b[SB_EPOCH0].at % 8 == 0 && b[SB_LEN].at % 4 == 0, AT);
#undef AT
                    }
}

// ---- the chunks of a span: what the launchers computed (spb = 16; if (ceil(span / spb) > 32768) spb = ceil(span / 32768);
// grid.y = ceil(span / spb)), and what a launch needs of them
static void check_chunks() {
    auto parent = [](int64_t span, int64_t *grid_y) {
        int64_t spb = 16;
        if ((span + spb - 1) / spb > 32768) spb = (span + 32767) / 32768;
        *grid_y = (span + spb - 1) / spb;
        return spb;
    };
    auto one = [&](int64_t span) {
        const SeriesChunks ch = series_chunks(span);
        const int64_t spb = ch.samples_per_block, gy = ch.grid_y;
        int64_t want_gy = 0;
        const int64_t want_spb = parent(span, &want_gy);
        CHECK(spb == want_spb && gy == want_gy, "span %lld: %lld x %lld, the launchers had %lld x %lld", (long long)span, (long long)gy,
              (long long)spb, (long long)want_gy, (long long)want_spb);
        CHECK(gy >= 1 && gy <= 32768, "span %lld: grid.y = %lld", (long long)span, (long long)gy);
        CHECK(gy * spb >= span, "span %lld: %lld x %lld leaves samples out", (long long)span, (long long)gy, (long long)spb);
        CHECK((gy - 1) * spb < span, "span %lld: %lld x %lld has an empty chunk", (long long)span, (long long)gy, (long long)spb);
        CHECK(span > 16 * 32768 || spb == 16, "span %lld: spb = %lld", (long long)span, (long long)spb);
        CHECK(span <= 16 * 32768 || spb > 16, "span %lld: spb = %lld", (long long)span, (long long)spb);
    };
    const int64_t seam = 16 * 32768, top = 2147483647LL;
    for (int64_t span : {(int64_t)1, (int64_t)15, (int64_t)16, (int64_t)17, seam, seam + 1, top}) one(span);
    for (int64_t span = 1; span <= 4096; ++span) one(span);
    for (int64_t span = seam - 4096; span <= seam + 4096; ++span) one(span);
    for (int64_t k = 17; k <= 40; ++k)   // the seams between spb = k - 1 and spb = k
        for (int64_t span = (k - 1) * 32768 - 40; span <= (k - 1) * 32768 + 40; ++span) one(span);
    for (int64_t span = top - 70000; span <= top; ++span) one(span);
    for (int64_t span = 1; span <= top - 999983; span += 999983) one(span);
}

int main(int argc, char **argv) {
    if (argc < 2) { std::printf("usage: series_host_check REFUSALS_OUT\n"); return 2; }
    std::FILE *f = std::fopen(argv[1], "w");
    if (!f) { std::printf("cannot write %s\n", argv[1]); return 2; }
    series_refusal_cases<Header>(f);
    std::fclose(f);
    check_block();
    check_chunks();
    if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
    std::printf("ok\n");
    return 0;
}
