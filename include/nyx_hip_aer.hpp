// nyx_hip_aer.hpp — thin C++17 wrapper of include/nyx_hip_aer.h, beside nyx_hip_groundtrack.hpp: what up to sixteen ground
// stations see of a TrajBatch (`GroundStation::azimuth_elevation_of` for every run and sample, up to eight parameters per launch).
#pragma once
#include <initializer_list>
#include <limits>
#include <stdexcept>
#include <vector>

#include "nyx_hip.hpp"
#include "nyx_hip_aer.h"

namespace nyx {

// The body-fixed frame the stations stand in: an IAU orientation of the trajectories' centre with its ellipsoid.
struct StationFrame {
    nyx_hip_rotation_t rotation{};    // NYX_HIP_ROT_IAU
    double eq_radius_km = 0.0;        // > 0
    double flattening = 0.0;          // [0, 1)
    bool rotating = true;             // false: identity orientation, the stations are at rest in the inertial frame
};

// values[((s * n_params + p) * capacity + k) * n + i]: parameter p of sample k of run i seen from station s; len[i] samples
// produced, the same for every station (NaN from there on)
struct AerSeries {
    int64_t n = 0, capacity = 0, step_ns = 0;
    std::vector<nyx_hip_station_t> stations;
    std::vector<nyx_hip_aer_param> params;
    std::vector<double> values;
    std::vector<int32_t> len;
    double at(size_t s, size_t p, int64_t k, int64_t i) const {
        return values[((s * params.size() + p) * (size_t)capacity + (size_t)k) * (size_t)n + (size_t)i];
    }
};

// `every(step)` of every run of `traj` seen from `stations` in `frame`; with `windowed`, `every_between(step, start, end)`.
inline AerSeries traj_aer(GpuPropagator &prop, TrajBatch &traj, const StationFrame &frame, const std::vector<nyx_hip_station_t> &stations,
                          std::initializer_list<nyx_hip_aer_param> params, int64_t step_ns, int64_t capacity, bool windowed = false,
                          int64_t start_ns = 0, int64_t end_ns = 0) {
    if (params.size() < 1 || params.size() > NYX_HIP_MAX_AER_PARAMS) throw std::invalid_argument("traj_aer: 1 .. 8 parameters per call");
    if (stations.size() < 1 || stations.size() > NYX_HIP_MAX_STATIONS) throw std::invalid_argument("traj_aer: 1 .. 16 stations per call");
    if (capacity < 1) throw std::invalid_argument("traj_aer: capacity must be >= 1");
    AerSeries out;
    out.n = traj.size();
    out.capacity = capacity;
    out.step_ns = step_ns;
    out.stations = stations;
    out.params.assign(params.begin(), params.end());
    out.values.assign(stations.size() * params.size() * (size_t)capacity * (size_t)out.n, std::numeric_limits<double>::quiet_NaN());
    out.len.assign((size_t)out.n, 0);
    nyx_hip_aer_query_t q{};
    q.n_params = (int32_t)params.size();
    q.has_window = windowed ? 1 : 0;
    int k = 0;
    for (nyx_hip_aer_param p : params) q.param[k++] = (int32_t)p;
    q.step_ns = step_ns;
    q.start_ns = start_ns;
    q.end_ns = end_ns;
    q.has_frame = frame.rotating ? 1 : 0;
    q.frame_eq_radius_km = frame.eq_radius_km;
    q.frame_flattening = frame.flattening;
    q.frame = frame.rotation;
    q.n_stations = (int32_t)stations.size();
    for (size_t s = 0; s < stations.size(); ++s) q.stations[s] = stations[s];
    nyx_hip_traj_t vi = traj.view();
    if (nyx_hip_traj_aer(prop.raw(), &vi, out.n, &q, capacity, out.values.data(), out.len.data()) != NYX_HIP_RC_OK)
        throw std::runtime_error(nyx_hip_last_error());
    return out;
}

}  // namespace nyx
