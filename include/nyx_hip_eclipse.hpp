// nyx_hip_eclipse.hpp — thin C++17 wrapper of include/nyx_hip_eclipse.h, beside nyx_hip_aer.hpp: the eclipse history of a TrajBatch
// (`ShadowModel::compute` for every run and sample, up to eight parameters per launch).
#pragma once
#include <limits>
#include <stdexcept>
#include <utility>
#include <vector>

#include "nyx_hip.hpp"
#include "nyx_hip_eclipse.h"

namespace nyx {

// The light source and the bodies that can hide it, each by its chain over the CONTEXT's segments and its mean radius.
struct ShadowModel {
    nyx_hip_ecl_body_t light{};                  // n_chain 1 .. 4
    std::vector<nyx_hip_ecl_body_t> bodies;      // 1 .. 8; n_chain 0 = the integration centre itself
};

// a parameter and, for the per-body ones (>= NYX_HIP_ECL_BODY_OCCULTATION), the index of its body in ShadowModel::bodies
using EclipseParam = std::pair<nyx_hip_ecl_param, int32_t>;

// values[(p * capacity + k) * n + i]: parameter p of sample k of run i; len[i] samples produced (NaN from there on)
struct EclipseSeries {
    int64_t n = 0, capacity = 0, step_ns = 0;
    std::vector<EclipseParam> params;
    std::vector<double> values;
    std::vector<int32_t> len;
    double at(size_t p, int64_t k, int64_t i) const { return values[(p * (size_t)capacity + (size_t)k) * (size_t)n + (size_t)i]; }
};

// `every(step)` of every run of `traj` under `model`; with `windowed`, `every_between(step, start, end)`.
inline EclipseSeries traj_eclipse(GpuPropagator &prop, TrajBatch &traj, const ShadowModel &model, const std::vector<EclipseParam> &params,
                                  int64_t step_ns, int64_t capacity, bool windowed = false, int64_t start_ns = 0, int64_t end_ns = 0) {
    if (params.size() < 1 || params.size() > NYX_HIP_MAX_ECL_PARAMS) throw std::invalid_argument("traj_eclipse: 1 .. 8 parameters per call");
    if (model.bodies.size() < 1 || model.bodies.size() > NYX_HIP_MAX_ECL_BODIES) throw std::invalid_argument("traj_eclipse: 1 .. 8 shadow bodies per call");
    if (capacity < 1) throw std::invalid_argument("traj_eclipse: capacity must be >= 1");
    EclipseSeries out;
    out.n = traj.size();
    out.capacity = capacity;
    out.step_ns = step_ns;
    out.params = params;
    out.values.assign(params.size() * (size_t)capacity * (size_t)out.n, std::numeric_limits<double>::quiet_NaN());
    out.len.assign((size_t)out.n, 0);
    nyx_hip_ecl_query_t q{};
    q.n_params = (int32_t)params.size();
    q.has_window = windowed ? 1 : 0;
    for (size_t k = 0; k < params.size(); ++k) { q.param[k] = (int32_t)params[k].first; q.param_body[k] = params[k].second; }
    q.step_ns = step_ns;
    q.start_ns = start_ns;
    q.end_ns = end_ns;
    q.light = model.light;
    q.n_bodies = (int32_t)model.bodies.size();
    for (size_t b = 0; b < model.bodies.size(); ++b) q.bodies[b] = model.bodies[b];
    nyx_hip_traj_t vi = traj.view();
    if (nyx_hip_traj_eclipse(prop.raw(), &vi, out.n, &q, capacity, out.values.data(), out.len.data()) != NYX_HIP_RC_OK)
        throw std::runtime_error(nyx_hip_last_error());
    return out;
}

}  // namespace nyx
