// nyx_hip_link.hpp — thin C++17 wrapper of include/nyx_hip_link.h, beside nyx_hip_ric.hpp and nyx_hip_eclipse.hpp: the range, the
// Doppler and the line of sight from a transmitter trajectory to every run of a TrajBatch (what
// `InterlinkTxSpacecraft::measure_instantaneous` forms for one pair, for every run and sample, up to eight parameters per launch).
#pragma once
#include <limits>
#include <stdexcept>
#include <vector>

#include "nyx_hip.hpp"
#include "nyx_hip_link.h"

namespace nyx {

// A body that can block the line: its chain over the CONTEXT's segments (n_chain 0 = the integration centre itself) and its radius.
struct LinkBody {
    int32_t n_chain = 0;
    int32_t chain_segment[NYX_HIP_MAX_CHAIN] = {0, 0, 0, 0};
    int32_t chain_sign[NYX_HIP_MAX_CHAIN] = {1, 1, 1, 1};
    double mean_radius_km = 0.0;
};

// one requested value: an enum nyx_hip_link_param and, for the per-body ones, the index into the bodies
struct LinkParam {
    int32_t param = NYX_HIP_LNK_RANGE;
    int32_t body = 0;
};

// values[(p * capacity + k) * n + i]: parameter p of sample k of run i, taken at epoch0_ns[i] + k * step_ns; len[i] samples
// produced (NaN from there on)
struct LinkSeries {
    int64_t n = 0, capacity = 0, step_ns = 0;
    std::vector<LinkParam> params;
    std::vector<double> values;
    std::vector<int32_t> len;
    std::vector<int64_t> epoch0_ns;
    double at(size_t p, int64_t k, int64_t i) const { return values[(p * (size_t)capacity + (size_t)k) * (size_t)n + (size_t)i]; }
};

// every run of `traj` (the receivers) seen from `ref` (the transmitter: one trajectory, or one per run) every `step_ns` over the
// overlap of the two spans; with `windowed`, clamped to [start_ns, end_ns]
inline LinkSeries traj_link(GpuPropagator &prop, TrajBatch &traj, TrajBatch &ref, const std::vector<LinkBody> &bodies,
                            const std::vector<LinkParam> &params, int64_t step_ns, int64_t capacity, bool windowed = false, int64_t start_ns = 0,
                            int64_t end_ns = 0) {
    if (params.size() < 1 || params.size() > NYX_HIP_MAX_LINK_PARAMS) throw std::invalid_argument("traj_link: 1 .. 8 parameters per call");
    if (bodies.size() > NYX_HIP_MAX_LINK_BODIES) throw std::invalid_argument("traj_link: at most 8 bodies per call");
    if (capacity < 1) throw std::invalid_argument("traj_link: capacity must be >= 1");
    LinkSeries out;
    out.n = traj.size();
    out.capacity = capacity;
    out.step_ns = step_ns;
    out.params = params;
    out.values.assign(params.size() * (size_t)capacity * (size_t)out.n, std::numeric_limits<double>::quiet_NaN());
    out.len.assign((size_t)out.n, 0);
    out.epoch0_ns.assign((size_t)out.n, 0);
    nyx_hip_link_query_t q{};
    q.n_params = (int32_t)params.size();
    for (size_t k = 0; k < params.size(); ++k) { q.param[k] = params[k].param; q.param_body[k] = params[k].body; }
    q.has_window = windowed ? 1 : 0;
    q.step_ns = step_ns;
    q.start_ns = start_ns;
    q.end_ns = end_ns;
    q.n_bodies = (int32_t)bodies.size();
    for (size_t b = 0; b < bodies.size(); ++b) {
        q.bodies[b].n_chain = bodies[b].n_chain;
        for (int k = 0; k < NYX_HIP_MAX_CHAIN; ++k) { q.bodies[b].chain_segment[k] = bodies[b].chain_segment[k]; q.bodies[b].chain_sign[k] = bodies[b].chain_sign[k]; }
        q.bodies[b].mean_radius_km = bodies[b].mean_radius_km;
    }
    nyx_hip_traj_t vi = traj.view(), vr = ref.view();
    if (nyx_hip_traj_link(prop.raw(), &vi, out.n, &vr, ref.size(), &q, capacity, out.values.data(), out.len.data(), out.epoch0_ns.data()) != NYX_HIP_RC_OK)
        throw std::runtime_error(nyx_hip_last_error());
    return out;
}

}  // namespace nyx
