// nyx_hip_reports.hpp — thin C++17 wrapper of include/nyx_hip_reports.h, beside nyx_hip.hpp: the fused device reports of a
// TrajBatch (`Results::every_value_of` / `every_value_of_between` for up to eight state parameters per launch).
#pragma once
#include <initializer_list>
#include <limits>
#include <stdexcept>
#include <vector>

#include "nyx_hip.hpp"
#include "nyx_hip_reports.h"

namespace nyx {

// values[(p * capacity + k) * n + i]: parameter p of sample k of run i; len[i] samples produced (NaN from there on)
struct ValueSeries {
    int64_t n = 0, capacity = 0, step_ns = 0;
    std::vector<nyx_hip_state_param> params;
    std::vector<double> values;
    std::vector<int32_t> len;
    double at(size_t p, int64_t k, int64_t i) const { return values[(p * (size_t)capacity + (size_t)k) * (size_t)n + (size_t)i]; }
};

// `every(step)` of every run of `traj`; with `windowed`, `every_between(step, start, end)`.  mu <= 0: the context's central body.
inline ValueSeries traj_values(GpuPropagator &prop, TrajBatch &traj, std::initializer_list<nyx_hip_state_param> params, int64_t step_ns,
                               int64_t capacity, bool windowed = false, int64_t start_ns = 0, int64_t end_ns = 0, double mu_km3_s2 = 0.0) {
    if (params.size() < 1 || params.size() > NYX_HIP_MAX_REPORT_PARAMS) throw std::invalid_argument("traj_values: 1 .. 8 parameters per call");
    if (capacity < 1) throw std::invalid_argument("traj_values: capacity must be >= 1");
    ValueSeries out;
    out.n = traj.size();
    out.capacity = capacity;
    out.step_ns = step_ns;
    out.params.assign(params.begin(), params.end());
    out.values.assign(params.size() * (size_t)capacity * (size_t)out.n, std::numeric_limits<double>::quiet_NaN());
    out.len.assign((size_t)out.n, 0);
    nyx_hip_values_query_t q{};
    q.n_params = (int32_t)params.size();
    q.has_window = windowed ? 1 : 0;
    int k = 0;
    for (nyx_hip_state_param p : params) q.param[k++] = (int32_t)p;
    q.step_ns = step_ns;
    q.start_ns = start_ns;
    q.end_ns = end_ns;
    q.mu_km3_s2 = mu_km3_s2;
    nyx_hip_traj_t vi = traj.view();
    if (nyx_hip_traj_values(prop.raw(), &vi, out.n, &q, capacity, out.values.data(), out.len.data()) != NYX_HIP_RC_OK)
        throw std::runtime_error(nyx_hip_last_error());
    return out;
}

}  // namespace nyx
