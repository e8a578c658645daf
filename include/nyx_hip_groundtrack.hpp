// nyx_hip_groundtrack.hpp — thin C++17 wrapper of include/nyx_hip_groundtrack.h, beside nyx_hip_reports.hpp: the ground
// tracks of a TrajBatch (`Traj::to_groundtrack_parquet` without the file, for up to eight parameters per launch).
#pragma once
#include <initializer_list>
#include <limits>
#include <stdexcept>
#include <vector>

#include "nyx_hip.hpp"
#include "nyx_hip_groundtrack.h"

namespace nyx {

// The body-fixed frame of a ground track: an IAU orientation of the trajectories' centre with its ellipsoid.
struct GroundFrame {
    nyx_hip_rotation_t rotation{};    // NYX_HIP_ROT_IAU
    double eq_radius_km = 0.0;        // > 0 for Latitude / Height
    double flattening = 0.0;          // [0, 1)
    bool rotating = true;             // false: identity orientation, the values are taken on the inertial state
};

// values[(p * capacity + k) * n + i]: parameter p of sample k of run i; len[i] samples produced (NaN from there on)
struct GroundTrackSeries {
    int64_t n = 0, capacity = 0, step_ns = 0;
    std::vector<nyx_hip_gt_param> params;
    std::vector<double> values;
    std::vector<int32_t> len;
    double at(size_t p, int64_t k, int64_t i) const { return values[(p * (size_t)capacity + (size_t)k) * (size_t)n + (size_t)i]; }
};

// `every(step)` of every run of `traj` in `frame`; with `windowed`, `every_between(step, start, end)`.
inline GroundTrackSeries traj_ground_track(GpuPropagator &prop, TrajBatch &traj, const GroundFrame &frame,
                                           std::initializer_list<nyx_hip_gt_param> params, int64_t step_ns, int64_t capacity,
                                           bool windowed = false, int64_t start_ns = 0, int64_t end_ns = 0) {
    if (params.size() < 1 || params.size() > NYX_HIP_MAX_GT_PARAMS) throw std::invalid_argument("traj_ground_track: 1 .. 8 parameters per call");
    if (capacity < 1) throw std::invalid_argument("traj_ground_track: capacity must be >= 1");
    GroundTrackSeries out;
    out.n = traj.size();
    out.capacity = capacity;
    out.step_ns = step_ns;
    out.params.assign(params.begin(), params.end());
    out.values.assign(params.size() * (size_t)capacity * (size_t)out.n, std::numeric_limits<double>::quiet_NaN());
    out.len.assign((size_t)out.n, 0);
    nyx_hip_gt_query_t q{};
    q.n_params = (int32_t)params.size();
    q.has_window = windowed ? 1 : 0;
    int k = 0;
    for (nyx_hip_gt_param p : params) q.param[k++] = (int32_t)p;
    q.step_ns = step_ns;
    q.start_ns = start_ns;
    q.end_ns = end_ns;
    q.has_frame = frame.rotating ? 1 : 0;
    q.frame_eq_radius_km = frame.eq_radius_km;
    q.frame_flattening = frame.flattening;
    q.frame = frame.rotation;
    nyx_hip_traj_t vi = traj.view();
    if (nyx_hip_traj_ground_track(prop.raw(), &vi, out.n, &q, capacity, out.values.data(), out.len.data()) != NYX_HIP_RC_OK)
        throw std::runtime_error(nyx_hip_last_error());
    return out;
}

}  // namespace nyx
