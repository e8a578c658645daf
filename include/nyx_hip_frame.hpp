// nyx_hip_frame.hpp — thin C++17 wrapper of include/nyx_hip_frame.h, beside nyx_hip_eclipse.hpp: a TrajBatch seen from another body
// (`Traj::to_frame` then the elements and the B-plane about that body, for every run and sample, up to eight parameters per launch).
#pragma once
#include <limits>
#include <stdexcept>
#include <vector>

#include "nyx_hip.hpp"
#include "nyx_hip_frame.h"

namespace nyx {

// The centre the runs are seen from: its chain over the CONTEXT's segments (n_chain 0 = the integration centre itself) and its mu.
struct FrameTarget {
    int32_t n_chain = 0;
    int32_t chain_segment[NYX_HIP_MAX_CHAIN] = {0, 0, 0, 0};
    int32_t chain_sign[NYX_HIP_MAX_CHAIN] = {1, 1, 1, 1};
    double mu_km3_s2 = 0.0;
};

// values[(p * capacity + k) * n + i]: parameter p of sample k of run i; len[i] samples produced (NaN from there on)
struct FrameSeries {
    int64_t n = 0, capacity = 0, step_ns = 0;
    std::vector<int32_t> params;   // enum nyx_hip_frame_param (0 .. 18: enum nyx_hip_state_param)
    std::vector<double> values;
    std::vector<int32_t> len;
    double at(size_t p, int64_t k, int64_t i) const { return values[(p * (size_t)capacity + (size_t)k) * (size_t)n + (size_t)i]; }
};

// `every(step)` of every run of `traj` about `target`; with `windowed`, `every_between(step, start, end)`.
inline FrameSeries traj_frame_values(GpuPropagator &prop, TrajBatch &traj, const FrameTarget &target, const std::vector<int32_t> &params,
                                     int64_t step_ns, int64_t capacity, bool windowed = false, int64_t start_ns = 0, int64_t end_ns = 0) {
    if (params.size() < 1 || params.size() > NYX_HIP_MAX_FRAME_PARAMS) throw std::invalid_argument("traj_frame_values: 1 .. 8 parameters per call");
    if (capacity < 1) throw std::invalid_argument("traj_frame_values: capacity must be >= 1");
    FrameSeries out;
    out.n = traj.size();
    out.capacity = capacity;
    out.step_ns = step_ns;
    out.params = params;
    out.values.assign(params.size() * (size_t)capacity * (size_t)out.n, std::numeric_limits<double>::quiet_NaN());
    out.len.assign((size_t)out.n, 0);
    nyx_hip_frame_query_t q{};
    q.n_params = (int32_t)params.size();
    q.has_window = windowed ? 1 : 0;
    for (size_t k = 0; k < params.size(); ++k) q.param[k] = params[k];
    q.step_ns = step_ns;
    q.start_ns = start_ns;
    q.end_ns = end_ns;
    q.n_chain = target.n_chain;
    for (int k = 0; k < NYX_HIP_MAX_CHAIN; ++k) { q.chain_segment[k] = target.chain_segment[k]; q.chain_sign[k] = target.chain_sign[k]; }
    q.mu_km3_s2 = target.mu_km3_s2;
    nyx_hip_traj_t vi = traj.view();
    if (nyx_hip_traj_frame_values(prop.raw(), &vi, out.n, &q, capacity, out.values.data(), out.len.data()) != NYX_HIP_RC_OK)
        throw std::runtime_error(nyx_hip_last_error());
    return out;
}

}  // namespace nyx
