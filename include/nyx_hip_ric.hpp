// nyx_hip_ric.hpp — thin C++17 wrapper of include/nyx_hip_ric.h, beside nyx_hip_reports.hpp: the RIC dispersions of a
// TrajBatch against a nominal trajectory (`Traj::ric_diff_to_parquet` for every run of an ensemble, and the per-sample sums
// of their mean and covariance).
#pragma once
#include <limits>
#include <stdexcept>
#include <vector>

#include "nyx_hip.hpp"
#include "nyx_hip_ric.h"

namespace nyx {

// values[(c * capacity + k) * n + i]: component c (dR dI dC dvR dvI dvC) of sample k of run i, taken at epoch0_ns[i] + k * step_ns;
// len[i] samples produced (NaN from there on); moments[k * 28 + q]: count, sum d[6], upper triangle of sum d d^T (empty unless asked for)
struct RicSeries {
    int64_t n = 0, capacity = 0, step_ns = 0;
    std::vector<double> values;
    std::vector<int32_t> len;
    std::vector<int64_t> epoch0_ns;
    std::vector<double> moments;
    double at(int c, int64_t k, int64_t i) const { return values[((size_t)c * (size_t)capacity + (size_t)k) * (size_t)n + (size_t)i]; }
    double count(int64_t k) const { return moments[(size_t)k * NYX_HIP_RIC_MOMENTS]; }
};

struct RicOptions {
    bool frame_of_reference = true;   // the frame of the nominal; false: of each run (the reference's self.ric_difference(&other))
    bool transport = true;
    int smooth_window = 5;            // the reference's median filter; 0 or 1: none
    bool moments = false;
    bool windowed = false;
    int64_t start_ns = 0, end_ns = 0;
};

// every run of `traj` against `ref` (one trajectory, or one per run) every `step_ns` over the overlap of the two spans
inline RicSeries traj_ric_diff(GpuPropagator &prop, TrajBatch &traj, TrajBatch &ref, int64_t step_ns, int64_t capacity, const RicOptions &opt = RicOptions()) {
    if (capacity < 1) throw std::invalid_argument("traj_ric_diff: capacity must be >= 1");
    RicSeries out;
    out.n = traj.size();
    out.capacity = capacity;
    out.step_ns = step_ns;
    out.values.assign(6 * (size_t)capacity * (size_t)out.n, std::numeric_limits<double>::quiet_NaN());
    out.len.assign((size_t)out.n, 0);
    out.epoch0_ns.assign((size_t)out.n, 0);
    if (opt.moments) out.moments.assign((size_t)capacity * NYX_HIP_RIC_MOMENTS, 0.0);
    nyx_hip_ric_query_t q{};
    q.step_ns = step_ns;
    q.has_window = opt.windowed ? 1 : 0;
    q.start_ns = opt.start_ns;
    q.end_ns = opt.end_ns;
    q.frame_of = opt.frame_of_reference ? 1 : 0;
    q.transport = opt.transport ? 1 : 0;
    q.smooth_window = opt.smooth_window;
    nyx_hip_traj_t vi = traj.view(), vr = ref.view();
    if (nyx_hip_traj_ric_diff(prop.raw(), &vi, out.n, &vr, ref.size(), &q, capacity, out.values.data(), out.len.data(), out.epoch0_ns.data(),
                              opt.moments ? out.moments.data() : nullptr) != NYX_HIP_RC_OK)
        throw std::runtime_error(nyx_hip_last_error());
    return out;
}

}  // namespace nyx
