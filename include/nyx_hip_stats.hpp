// nyx_hip_stats.hpp — thin C++17 wrapper of include/nyx_hip_stats.h, beside nyx_hip_link.hpp and its siblings: the statistics over
// the runs of a values block of any series report (extremes, the sums behind mean and sigma, exact quantiles), and the fused
// entry that runs a report and the reduction back to back so that only the statistics come back.
#pragma once
#include <cmath>
#include <stdexcept>
#include <vector>

#include "nyx_hip.hpp"
#include "nyx_hip_stats.h"

namespace nyx {

// stats[(r * capacity + k) * (NYX_HIP_STAT_FIXED + n_probs) + s]: column s (enum nyx_hip_stat, then one per probability) of row r,
// sample k; len / epoch0_ns are filled by the fused entry only
struct SeriesStats {
    int64_t rows = 0, capacity = 0;
    std::vector<double> probs;
    std::vector<double> stats;
    std::vector<int32_t> len;
    std::vector<int64_t> epoch0_ns;
    size_t columns() const { return NYX_HIP_STAT_FIXED + probs.size(); }
    double at(int64_t r, int64_t k, size_t s) const { return stats[((size_t)r * (size_t)capacity + (size_t)k) * columns() + s]; }
    double quantile(int64_t r, int64_t k, size_t j) const { return at(r, k, NYX_HIP_STAT_FIXED + j); }
    // derived: over the finite values; NaN where there are too few
    double mean(int64_t r, int64_t k) const {
        const double n = at(r, k, NYX_HIP_STAT_FINITE);
        return n > 0 ? at(r, k, NYX_HIP_STAT_SHIFT) + at(r, k, NYX_HIP_STAT_SUM) / n : std::nan("");
    }
    double variance(int64_t r, int64_t k) const {
        const double n = at(r, k, NYX_HIP_STAT_FINITE), s = at(r, k, NYX_HIP_STAT_SUM);
        return n > 1 ? (at(r, k, NYX_HIP_STAT_SUMSQ) - s * s / n) / (n - 1) : std::nan("");
    }
};

inline nyx_hip_stats_query_t stats_query(const std::vector<double> &probs) {
    if (probs.size() > NYX_HIP_MAX_STAT_PROBS) throw std::invalid_argument("series_stats: at most 8 probabilities per call");
    nyx_hip_stats_query_t q{};
    q.n_probs = (int32_t)probs.size();
    for (size_t j = 0; j < probs.size(); ++j) q.prob[j] = probs[j];
    return q;
}

// a block values[rows][capacity][n] on the host with its len[n]; `status` (n entries, or null) leaves the runs with status != 0 out
inline SeriesStats series_stats(GpuPropagator &prop, const double *values, const int32_t *len, const int32_t *status, int64_t rows, int64_t capacity,
                                int64_t n, const std::vector<double> &probs) {
    SeriesStats out;
    out.rows = rows;
    out.capacity = capacity;
    out.probs = probs;
    const nyx_hip_stats_query_t q = stats_query(probs);
    out.stats.assign((size_t)rows * (size_t)capacity * out.columns(), 0.0);
    if (nyx_hip_series_stats(prop.raw(), values, len, status, rows, capacity, n, &q, out.stats.data()) != NYX_HIP_RC_OK)
        throw std::runtime_error(nyx_hip_last_error());
    return out;
}

// the report `kind` (enum nyx_hip_series_kind) with its query `q` over the runs of `traj` (`ref`: the second batch of LINK and RIC,
// else null), reduced on the device; `rows` as the header gives them for that kind
template <typename Query>
inline SeriesStats traj_series_stats(GpuPropagator &prop, int32_t kind, TrajBatch &traj, TrajBatch *ref, const Query &q, int64_t rows, int64_t capacity,
                                     const std::vector<double> &probs, const int32_t *status = nullptr) {
    SeriesStats out;
    out.rows = rows;
    out.capacity = capacity;
    out.probs = probs;
    const nyx_hip_stats_query_t sq = stats_query(probs);
    const int64_t n = traj.size();
    out.stats.assign((size_t)rows * (size_t)capacity * out.columns(), 0.0);
    out.len.assign((size_t)n, 0);
    if (ref) out.epoch0_ns.assign((size_t)n, 0);
    nyx_hip_traj_t vi = traj.view(), vr{};
    if (ref) vr = ref->view();
    if (nyx_hip_traj_series_stats(prop.raw(), kind, &vi, n, ref ? &vr : nullptr, ref ? ref->size() : 0, &q, (int64_t)sizeof(Query), capacity, status, &sq,
                                  out.stats.data(), out.len.data(), ref ? out.epoch0_ns.data() : nullptr) != NYX_HIP_RC_OK)
        throw std::runtime_error(nyx_hip_last_error());
    return out;
}

}  // namespace nyx
