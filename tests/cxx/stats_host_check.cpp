// stats_host_check.cpp - the host side of the statistics entries (nyx_amd/csrc/stats_host.h: what they refuse, the rows and the query
// size of every kind, the device block) and THE KERNEL'S OWN per-value code compiled for the host (nyx_amd/csrc/stats_dev.h: the key
// map, who is held, the quantile formula, the summation order) as a stand-alone program: g++ only, no HIP, no GPU.
//   stats_host_check <input>   reads blocks (rows capacity n n_probs / probs / len / status / values, doubles as hex floats), prints per
//                              (row, sample) the 10 + n_probs columns with %a, then the table of refusals as "rc|message" lines.
// The selection here is a std::sort of the keys: rank j of ALL n keys, as the kernel selects it.  tests/test_stats_host_cxx.py holds
// the output to nyx_amd/stats.py.
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../nyx_amd/csrc/stats_dev.h"
#include "../../nyx_amd/csrc/stats_host.h"

static double read_double(FILE *f) {
    char word[64];
    if (std::fscanf(f, "%63s", word) != 1) { std::fprintf(stderr, "short input\n"); std::exit(2); }
    return std::strtod(word, nullptr);
}
static long long read_int(FILE *f) {
    long long v;
    if (std::fscanf(f, "%lld", &v) != 1) { std::fprintf(stderr, "short input\n"); std::exit(2); }
    return v;
}

static void one_sample(const double *row, const int32_t *len, const int32_t *status, int64_t capacity, int64_t k, int32_t n,
                       const nyx_hip_stats_query_t &q, double *out) {
    std::vector<uint64_t> key((size_t)n);
    int held = 0, count = 0, finite = 0, first = -1, imin = -1, imax = -1;
    uint64_t kmin = STAT_KEY_OUT, kmax = 0;
    for (int32_t i = 0; i < n; ++i) {
        const bool h = stat_held(len, status, capacity, k, i);
        key[(size_t)i] = stat_key_of(row[i], h);
        held += h ? 1 : 0;
        if (key[(size_t)i] == STAT_KEY_OUT) continue;
        ++count;
        if (stat_key_finite(key[(size_t)i])) { ++finite; if (first < 0) first = i; }
        if (key[(size_t)i] < kmin) { kmin = key[(size_t)i]; imin = i; }
        if (key[(size_t)i] > kmax) { kmax = key[(size_t)i]; imax = i; }
    }
    const double shift = first >= 0 ? row[first] : 0.0, nan = stat_double(STAT_NAN_BITS);
    double sum, sumsq;
    stat_ordered_sums(key.data(), n, shift, &sum, &sumsq);
    out[NYX_HIP_STAT_HELD] = held; out[NYX_HIP_STAT_COUNT] = count; out[NYX_HIP_STAT_FINITE] = finite;
    out[NYX_HIP_STAT_MIN] = count ? stat_unkey(kmin) : nan; out[NYX_HIP_STAT_MAX] = count ? stat_unkey(kmax) : nan;
    out[NYX_HIP_STAT_ARGMIN] = count ? imin : -1; out[NYX_HIP_STAT_ARGMAX] = count ? imax : -1;
    out[NYX_HIP_STAT_SHIFT] = shift; out[NYX_HIP_STAT_SUM] = sum; out[NYX_HIP_STAT_SUMSQ] = sumsq;
    std::sort(key.begin(), key.end());
    for (int j = 0; j < q.n_probs; ++j) {
        if (!count) { out[NYX_HIP_STAT_FIXED + j] = nan; continue; }
        int32_t lo;
        const double g = stat_quantile_rank(count, q.prob[j], &lo);
        out[NYX_HIP_STAT_FIXED + j] = stat_quantile_value(stat_unkey(key[(size_t)lo]), g != 0.0 ? stat_unkey(key[(size_t)lo + 1]) : 0.0, g);
    }
}

static void show(const Refusal &r) { std::printf("%d|%s\n", r.rc, r.msg); }

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = std::fopen(argv[1], "r");
    if (!f) return 2;
    const long long blocks = read_int(f);
    for (long long b = 0; b < blocks; ++b) {
        const int64_t rows = read_int(f), capacity = read_int(f);
        const int32_t n = (int32_t)read_int(f);
        nyx_hip_stats_query_t q{};
        q.n_probs = (int32_t)read_int(f);
        const int has_status = (int)read_int(f);
        for (int j = 0; j < q.n_probs; ++j) q.prob[j] = read_double(f);
        std::vector<int32_t> len((size_t)n), status((size_t)n);
        for (auto &v : len) v = (int32_t)read_int(f);
        for (auto &v : status) v = (int32_t)read_int(f);
        std::vector<double> values((size_t)rows * (size_t)capacity * (size_t)n);
        for (auto &v : values) v = read_double(f);
        std::vector<double> out((size_t)(NYX_HIP_STAT_FIXED + q.n_probs));
        if (Refusal r = check_series_stats((const nyx_hip_ctx *)1, values.data(), len.data(), rows, capacity, n, &q, out.data())) { show(r); return 1; }
        for (int64_t r = 0; r < rows; ++r)
            for (int64_t k = 0; k < capacity; ++k) {
                one_sample(values.data() + (r * capacity + k) * n, len.data(), has_status ? status.data() : nullptr, capacity, k, n, q, out.data());
                for (double v : out) std::printf("%a ", v);
                std::printf("\n");
            }
    }
    std::fclose(f);

    // ---- the refusals, in the order tests/test_stats_host_cxx.py expects them
    std::printf("REFUSALS\n");
    const nyx_hip_ctx *ctx = (const nyx_hip_ctx *)1;
    double buf[4] = {0, 0, 0, 0};
    int32_t len[1] = {1};
    nyx_hip_stats_query_t ok{};
    ok.n_probs = 1; ok.prob[0] = 0.5;
    nyx_hip_stats_query_t bad = ok;
    show(check_series_stats(ctx, buf, len, 1, 1, 1, &ok, buf));
    show(check_series_stats(nullptr, buf, len, 1, 1, 1, &ok, buf));
    show(check_series_stats(ctx, buf, len, 1, 1, 1, nullptr, buf));
    bad.n_probs = 9; show(check_series_stats(ctx, buf, len, 1, 1, 1, &bad, buf));
    bad.n_probs = -1; show(check_series_stats(ctx, buf, len, 1, 1, 1, &bad, buf));
    bad = ok; bad.prob[0] = stat_double(STAT_NAN_BITS); show(check_series_stats(ctx, buf, len, 1, 1, 1, &bad, buf));
    bad.prob[0] = -0.25; show(check_series_stats(ctx, buf, len, 1, 1, 1, &bad, buf));
    bad.prob[0] = 1.25; show(check_series_stats(ctx, buf, len, 1, 1, 1, &bad, buf));
    show(check_series_stats(ctx, buf, len, 0, 1, 1, &ok, buf));
    show(check_series_stats(ctx, buf, len, 1, 0, 1, &ok, buf));
    show(check_series_stats(ctx, buf, len, 1, (int64_t)INT32_MAX + 1, 1, &ok, buf));
    show(check_series_stats(ctx, buf, len, 1, 1, -1, &ok, buf));
    show(check_series_stats(ctx, buf, len, 1, 1, 1, &ok, nullptr));
    show(check_series_stats(ctx, nullptr, len, 1, 1, 1, &ok, buf));
    show(check_series_stats(ctx, buf, nullptr, 1, 1, 1, &ok, buf));
    show(check_series_stats(ctx, nullptr, nullptr, 1, 1, 0, &ok, buf));   // (no run: no values needed)
    // the fused entry
    nyx_hip_traj_t traj{};
    nyx_hip_values_query_t vq{};
    nyx_hip_link_query_t lq{};
    show(check_traj_series_stats(ctx, NYX_HIP_SERIES_VALUES, &traj, nullptr, &vq, sizeof vq, &ok, buf, len));
    show(check_traj_series_stats(nullptr, NYX_HIP_SERIES_VALUES, &traj, nullptr, &vq, sizeof vq, &ok, buf, len));
    show(check_traj_series_stats(ctx, NYX_HIP_SERIES_COUNT, &traj, nullptr, &vq, sizeof vq, &ok, buf, len));
    show(check_traj_series_stats(ctx, NYX_HIP_SERIES_VALUES, nullptr, nullptr, &vq, sizeof vq, &ok, buf, len));
    show(check_traj_series_stats(ctx, NYX_HIP_SERIES_VALUES, &traj, nullptr, nullptr, sizeof vq, &ok, buf, len));
    show(check_traj_series_stats(ctx, NYX_HIP_SERIES_VALUES, &traj, nullptr, &vq, sizeof vq - 8, &ok, buf, len));
    show(check_traj_series_stats(ctx, NYX_HIP_SERIES_VALUES, &traj, &traj, &vq, sizeof vq, &ok, buf, len));
    show(check_traj_series_stats(ctx, NYX_HIP_SERIES_LINK, &traj, nullptr, &lq, sizeof lq, &ok, buf, len));
    show(check_traj_series_stats(ctx, NYX_HIP_SERIES_LINK, &traj, &traj, &lq, sizeof lq, &ok, buf, len));
    show(check_traj_series_stats(ctx, NYX_HIP_SERIES_VALUES, &traj, nullptr, &vq, sizeof vq, &bad, buf, len));
    show(check_traj_series_stats(ctx, NYX_HIP_SERIES_VALUES, &traj, nullptr, &vq, sizeof vq, &ok, nullptr, len));
    show(check_traj_series_stats(ctx, NYX_HIP_SERIES_VALUES, &traj, nullptr, &vq, sizeof vq, &ok, buf, nullptr));
    // rows and sizes of every kind, and the device block
    nyx_hip_aer_query_t aq{};
    aq.n_stations = 3; aq.n_params = 4;
    vq.n_params = 5;
    std::printf("rows %lld %lld %lld\n", (long long)series_kind_rows(NYX_HIP_SERIES_VALUES, &vq), (long long)series_kind_rows(NYX_HIP_SERIES_AER, &aq),
                (long long)series_kind_rows(NYX_HIP_SERIES_RIC, nullptr));
    for (int kind = 0; kind < NYX_HIP_SERIES_COUNT; ++kind) {
        SeriesKind kd;
        if (!series_kind(kind, &kd)) return 1;
        std::printf("kind %d %lld %d %s\n", kind, (long long)kd.query_size, (int)kd.with_ref, kd.name);
    }
    const Block<STB_PARTS> sb = stats_block(8, 91, 10000, 3, true);
    std::printf("block");
    for (int k : {STB_VALUES, STB_STATS, STB_LEN, STB_STATUS}) std::printf(" %zu %zu", sb[k].at, sb[k].bytes);
    std::printf(" %zu\n", sb.total);
    return 0;
}
