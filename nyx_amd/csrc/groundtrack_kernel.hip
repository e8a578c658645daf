// groundtrack_kernel.hip — ground tracks on the MI355X (gfx950): resample every trajectory of a batch (`Traj::every` /
// `Traj::every_between`, md/trajectory/traj.rs:148-162), express the interpolated state in an IAU-oriented body-fixed
// frame AT THE SAMPLE'S EPOCH and write ONLY the requested values - geodetic latitude, longitude, height, |r|, the
// declination, the body-fixed Cartesian state and the ground-relative speed (include/nyx_hip_groundtrack.h;
// `Traj::to_groundtrack_parquet`, md/trajectory/sc_traj.rs:131-155).  A sibling of report_kernel.hip.
//
// Mapping: as report_kernel.hip - lane <-> trajectory, a workgroup is ONE wave that owns 64 trajectories x a chunk of
// consecutive samples (grid.y walks the chunks), so the dense output is read and values[(p * capacity + k) * n + i] is
// written fully coalesced.  The interpolation is `traj_at` of traj_dev.h, the code nyx_traj_eval_kernel runs: the inertial
// state is bit-identical to what nyx_hip_traj_every returns for that epoch.
//
// Bound: FP64 VALU, by HRMINT's ~1 800 divisions per sample (traj_kernel.hip).  The frame block (`ev_to_frame` of
// event_dev.h, the code of the stop conditions: three sincos plus one per nutation-precession term, with the lane's own
// epoch) and the geodetic iteration (`ev_geodetic`: a sin, a sqrt and an atan2 per pass) start after the divided-difference
// tables are dead, so they do not add to the register peak of the interpolation.  Whether the frame is applied, and which
// shared intermediates (|r|, the geodetic pair) are built, is decided by kernel arguments: scalar branches, the same for
// every lane.
//
// The formulas are the ones of event_dev.h (sums of three left to right, a0 + a1 + a2), restated on the host by
// nyx_amd/groundtrack.py, which is what this kernel is tested against; compiled with -ffp-contract=off.

#include <hip/hip_runtime.h>

#include "../../include/nyx_hip_groundtrack.h"
#include "event_dev.h"
#include "groundtrack_args.h"
#include "series_host.h"   // series_chunks
#include "traj_dev.h"

namespace {

constexpr double GT_DEG = 180.0 / 3.14159265358979323846;

// The first and the count of the inclusive series of one trajectory (TimeSeries::inclusive(lo, hi, step))
DEVFN void gt_series(const GroundTrackArgs &a, const View &v, int64_t &lo, int64_t &count) {
    lo = 0;
    count = 0;
    if (v.len <= 0) return;
    lo = v.epoch[v.at(0)];
    int64_t hi = v.epoch[v.at(v.len - 1)];
    if (a.q.has_window) {
        lo = a.q.start_ns > lo ? a.q.start_ns : lo;
        hi = a.q.end_ns < hi ? a.q.end_ns : hi;
    }
    if (hi >= lo) count = (hi - lo) / a.q.step_ns + 1;
}

struct GtShared {  // what several parameters of one sample have in common
    double rmag, lat_deg, height_km;
};

// `param` is the same for every lane (a kernel argument): the chain below is a scalar branch
DEVFN double gt_value(int32_t param, const double y[6], const GtShared &s) {
    switch (param) {
    case NYX_HIP_GT_LATITUDE: return s.lat_deg;
    case NYX_HIP_GT_LONGITUDE: {  // NYX_HIP_EV_LONGITUDE_DEG; a negative angle below half an ulp of 360 would round to 360: it is 0
        const double deg = atan2(y[1], y[0]) * GT_DEG;
        const double w = deg < 0.0 ? deg + 360.0 : deg;
        return w >= 360.0 ? 0.0 : w;
    }
    case NYX_HIP_GT_HEIGHT: return s.height_km;
    case NYX_HIP_GT_RMAG: return s.rmag;
    case NYX_HIP_GT_DECLINATION: return asin(y[2] / s.rmag) * GT_DEG;
    case NYX_HIP_GT_X: return y[0];
    case NYX_HIP_GT_Y: return y[1];
    case NYX_HIP_GT_Z: return y[2];
    case NYX_HIP_GT_VX: return y[3];
    case NYX_HIP_GT_VY: return y[4];
    case NYX_HIP_GT_VZ: return y[5];
    case NYX_HIP_GT_VMAG: return sqrt(y[3] * y[3] + y[4] * y[4] + y[5] * y[5]);
    default: return __builtin_nan("");
    }
}

}  // namespace

// len[i] = the length of the inclusive series (the evaluation kernel lowers it to the first failing sample)
__global__ __launch_bounds__(256) void nyxgt_init_kernel(GroundTrackArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    int64_t lo, count;
    gt_series(a, make_view(a.src, a.n, i), lo, count);
    a.len[i] = count > INT32_MAX ? INT32_MAX : (int32_t)count;
}

// Every slot (p, k < capacity, i) is written here: the values of an interpolated sample, NaN otherwise (a sample that
// failed, or a slot beyond the series).
__global__ __launch_bounds__(LANES) void nyxgt_values_kernel(GroundTrackArgs a) {
    const int lane = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * LANES + lane;
    const bool live = i < a.n;
    const int64_t ii = live ? i : a.n - 1;  // idle lanes shadow a valid trajectory and store nothing
    const View v = make_view(a.src, a.n, ii);
    int64_t lo, count;
    gt_series(a, v, lo, count);
    const int64_t q0 = (int64_t)blockIdx.y * a.samples_per_block;
    const int64_t q_hi = q0 + a.samples_per_block < a.capacity ? q0 + a.samples_per_block : a.capacity;
    const int64_t q_end = count < q_hi ? count : q_hi;  // the samples of THIS trajectory in the chunk: [q0, q_end)
    const double qnan = __builtin_nan("");
    for (int64_t q = q0; __any(q < q_end); ++q) {
        // lanes past the end of their series ride along on their first epoch (the wave runs one instruction stream)
        const bool mine = live && q < q_end;
        const int64_t epoch = lo + (q < q_end ? q : 0) * a.q.step_ns;
        double s6[6], yf[6];
        const bool ok = traj_at(a.src, v, epoch, s6) == NYX_HIP_INTERP_OK;
        if (mine && !ok) atomicMin(&a.len[i], (int32_t)q);
        // the frame at the epoch of THIS lane's sample (has_frame is a kernel argument: a scalar branch)
        if (a.q.has_frame) {
            ev_to_frame(a.q, epoch, s6, yf);
        } else {
#pragma unroll
            for (int c = 0; c < 6; ++c) yf[c] = s6[c];
        }
        GtShared sh;
        if (a.need & GT_NEED_R) sh.rmag = sqrt(yf[0] * yf[0] + yf[1] * yf[1] + yf[2] * yf[2]);
        if (a.need & GT_NEED_GEODETIC) ev_geodetic(a.q.frame_eq_radius_km, a.q.frame_flattening, yf, sh.lat_deg, sh.height_km);
#pragma unroll 1   // (one copy of the parameter code; p and param[p] are scalars)
        for (int p = 0; p < a.q.n_params; ++p) {
            const double val = gt_value(a.q.param[p], yf, sh);
            if (mine) a.values[((int64_t)p * a.capacity + q) * a.n + i] = ok ? val : qnan;
        }
    }
    // the rest of the chunk lies beyond the series
    if (live)
        for (int64_t q = q_end > q0 ? q_end : q0; q < q_hi; ++q)
            for (int p = 0; p < a.q.n_params; ++p) a.values[((int64_t)p * a.capacity + q) * a.n + i] = qnan;
}

// The series of a trajectory ENDS at its first failing sample (traj_it.rs:39-61): what later chunks stored after it is
// blanked.  Trajectories without a failing sample (all of them, normally) have nothing to do here.
__global__ __launch_bounds__(256) void nyxgt_seal_kernel(GroundTrackArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    int64_t lo, count;
    gt_series(a, make_view(a.src, a.n, i), lo, count);
    const int64_t top = count < a.capacity ? count : a.capacity;
    const double qnan = __builtin_nan("");
    for (int64_t q = a.len[i]; q < top; ++q)
        for (int p = 0; p < a.q.n_params; ++p) a.values[((int64_t)p * a.capacity + q) * a.n + i] = qnan;
}

extern "C" hipError_t nyx_launch_ground_track(const GroundTrackArgs *args, hipStream_t stream) {
    GroundTrackArgs a = *args;
    if (a.n <= 0 || a.capacity <= 0) return hipSuccess;
    a.need = 0;
    for (int p = 0; p < a.q.n_params; ++p) a.need |= gt_param_needs(a.q.param[p]);
    const dim3 per_traj((unsigned)((a.n + 255) / 256));
    hipLaunchKernelGGL(nyxgt_init_kernel, per_traj, dim3(256), 0, stream, a);
    const SeriesChunks chunks = series_chunks(a.capacity);
    a.samples_per_block = chunks.samples_per_block;
    const dim3 grid((unsigned)((a.n + LANES - 1) / LANES), chunks.grid_y);
    hipLaunchKernelGGL(nyxgt_values_kernel, grid, dim3(LANES), 0, stream, a);
    hipLaunchKernelGGL(nyxgt_seal_kernel, per_traj, dim3(256), 0, stream, a);
    return hipGetLastError();
}
