// aer_kernel.hip — station views on the MI355X (gfx950): resample every trajectory of a batch (`Traj::every` /
// `Traj::every_between`, md/trajectory/traj.rs:148-162), express the interpolated state in an IAU-oriented body-fixed frame
// AT THE SAMPLE'S EPOCH and write, for every one of up to sixteen ground stations, ONLY the requested values - azimuth,
// elevation, range, range rate, the elevation above the station's mask, the visibility flag and the line of sight in the
// station's south-east-zenith triad (include/nyx_hip_aer.h; `GroundStation::azimuth_elevation_of`,
// od/ground_station/mod.rs:69-105).  A sibling of groundtrack_kernel.hip.
//
// Mapping: lane <-> trajectory as in groundtrack_kernel.hip; a workgroup is ONE wave that owns 64 trajectories x a tile of
// AER_TILE consecutive samples (grid.y walks the tiles), so the dense output is read and
// values[((s * n_params + p) * capacity + k) * n + i] is written fully coalesced.  The interpolation is `traj_at` of traj_dev.h,
// the code nyx_traj_eval_kernel runs.
//
// ONE interpolation and ONE frame rotation per sample serve ALL stations.  The bound is FP64 VALU, by HRMINT's ~1 800 divisions
// per sample (traj_kernel.hip); a station adds three dot products, a sqrt and, where asked for, an asin, an atan2 and a division.
// The constants of a station (its body-fixed position, its triad, its mask: aer_args.h, computed on the host) are kernel
// arguments indexed by the scalar loop counter - scalar loads, the same for every lane - and so are the branches on `need` and
// `param`; both loops (stations, parameters) are rolled.
//
// WHY TWO PASSES.  The straightforward shape - the station loop inside the sample loop, right after the frame - was built first
// and MISCOMPILED (hipcc 7.2): what is alive across `traj_at` (the first epoch of the lane's series, then the hoisted constants of
// asin / atan2) exceeds the 256 architectural VGPRs while HRMINT runs, and the register allocator parked it in AGPRs with
// v_accvgpr_write copies placed in the structurizer's "Flow" block of the LAST divergent branch before HRMINT (the century test
// of `ns_to_seconds`), BEFORE the exec mask is rejoined.  Every lane takes the other side of that branch, so the copies ran
// with an empty mask, the reload after HRMINT returned whatever an earlier wave had left in those AGPRs, and from the second
// interpolated sample of a wave on every epoch was garbage: NoInterpolationData, len[i] = 3.  The kernel therefore interpolates
// a tile first and parks the body-fixed states in LDS, and evaluates the stations in a second loop with NO loop around the two:
// nothing of the station block is alive while HRMINT runs, the first pass carries less than the ground-track kernel's, and the
// code object holds no such copy (checked on the ISA; tests/test_gpu_aer.py compares every sample).
//
// The formulas (sums of three left to right, a0 + a1 + a2) are restated on the host by nyx_amd/stations.py, which is what this
// kernel is tested against; compiled with -ffp-contract=off.

#include <hip/hip_runtime.h>

#include "../../include/nyx_hip_aer.h"
#include "aer_args.h"
#include "event_dev.h"
#include "series_host.h"   // kMaxChunks
#include "traj_dev.h"

namespace {

constexpr double AER_DEG = 180.0 / 3.14159265358979323846;
constexpr int AER_TILE = 8;   // samples a workgroup interpolates, parks and then evaluates

// The first and the count of the inclusive series of one trajectory (TimeSeries::inclusive(lo, hi, step))
DEVFN void aer_series(const AerArgs &a, const View &v, int64_t &lo, int64_t &count) {
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

struct AerShared {  // what several parameters of one (sample, station) have in common
    double rho_s, rho_e, rho_z, range, el_deg, az_deg, range_rate, mask_deg;
};

// `param` is the same for every lane (a kernel argument): the chain below is a scalar branch
DEVFN double aer_value(int32_t param, const AerShared &s) {
    switch (param) {
    case NYX_HIP_AER_AZIMUTH: return s.az_deg;
    case NYX_HIP_AER_ELEVATION: return s.el_deg;
    case NYX_HIP_AER_RANGE: return s.range;
    case NYX_HIP_AER_RANGE_RATE: return s.range_rate;
    case NYX_HIP_AER_ELEVATION_ABOVE_MASK: return s.el_deg - s.mask_deg;
    case NYX_HIP_AER_VISIBLE: return s.el_deg - s.mask_deg >= 0.0 ? 1.0 : 0.0;  // (a NaN elevation is not visible)
    case NYX_HIP_AER_RHO_S: return s.rho_s;
    case NYX_HIP_AER_RHO_E: return s.rho_e;
    case NYX_HIP_AER_RHO_Z: return s.rho_z;
    default: return __builtin_nan("");
    }
}

}  // namespace

// len[i] = the length of the inclusive series (the evaluation kernel lowers it to the first failing sample)
__global__ __launch_bounds__(256) void nyxaer_init_kernel(AerArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    int64_t lo, count;
    aer_series(a, make_view(a.src, a.n, i), lo, count);
    a.len[i] = count > INT32_MAX ? INT32_MAX : (int32_t)count;
}

// Every slot (s, p, k < capacity, i) of the tile is written here: the values of an interpolated sample, NaN otherwise (a sample
// that failed, or a slot beyond the series).  Two passes over the AER_TILE samples of the tile.  The first is the sample loop of
// the ground tracks without its value block: `traj_at`, the frame, and the body-fixed state parked in LDS - a column per lane,
// written and read by that lane alone, so the one wave of the workgroup needs no barrier.  The second walks the parked states:
// stations, then parameters.  What the station block keeps in registers (the polynomial constants of asin / atan2 above all) is
// therefore not alive while HRMINT runs, and the first pass is as light as the sibling's.
__global__ __launch_bounds__(LANES) void nyxaer_values_kernel(AerArgs a) {
    __shared__ double parked[AER_TILE][6][LANES];   // 24 KiB: four waves a CU keep their 160 KiB
    const int lane = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * LANES + lane;
    const bool live = i < a.n;
    const int64_t ii = live ? i : a.n - 1;  // idle lanes shadow a valid trajectory and store nothing
    const View v = make_view(a.src, a.n, ii);
    int64_t lo, count;
    aer_series(a, v, lo, count);
    const int64_t q0 = a.sample0 + (int64_t)blockIdx.y * AER_TILE;
    const int64_t q_hi = q0 + AER_TILE < a.capacity ? q0 + AER_TILE : a.capacity;
    const int64_t q_end = count < q_hi ? count : q_hi;  // the samples of THIS trajectory in the tile: [q0, q_end)
    const int64_t rows = (int64_t)a.q.n_stations * a.q.n_params;
    const double qnan = __builtin_nan("");
    uint32_t ok_bits = 0;   // bit t: sample q0 + t of this lane was interpolated
#pragma unroll 1
    for (int t = 0; t < AER_TILE && __any(q0 + t < q_end); ++t) {
        // lanes past the end of their series ride along on their first epoch (the wave runs one instruction stream)
        const int64_t q = q0 + t;
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
#pragma unroll
        for (int c = 0; c < 6; ++c) parked[t][c][lane] = yf[c];
        ok_bits |= (ok ? 1u : 0u) << t;
    }
#pragma unroll 1
    for (int t = 0; t < AER_TILE && __any(q0 + t < q_end); ++t) {
        const int64_t q = q0 + t;
        const bool mine = live && q < q_end;
        const bool ok = (ok_bits >> t) & 1u;
        double yf[6];
#pragma unroll
        for (int c = 0; c < 6; ++c) yf[c] = parked[t][c][lane];
#pragma unroll 1   // (one copy of the station code; s and the constants of station s are scalars)
        for (int s = 0; s < a.q.n_stations; ++s) {
            const AerStationConsts &c = a.st[s];
            const double rx = yf[0] - c.r_km[0], ry = yf[1] - c.r_km[1], rz = yf[2] - c.r_km[2];
            AerShared sh;
            sh.rho_s = rx * c.south[0] + ry * c.south[1] + rz * c.south[2];
            sh.rho_e = rx * c.east[0] + ry * c.east[1] + rz * c.east[2];
            sh.rho_z = rx * c.zenith[0] + ry * c.zenith[1] + rz * c.zenith[2];
            sh.range = sqrt(sh.rho_s * sh.rho_s + sh.rho_e * sh.rho_e + sh.rho_z * sh.rho_z);
            sh.mask_deg = c.mask_deg;
            sh.el_deg = sh.az_deg = sh.range_rate = qnan;
            if (a.need & AER_NEED_ELEVATION) sh.el_deg = asin(sh.rho_z / sh.range) * AER_DEG;
            if (a.need & AER_NEED_AZIMUTH) {  // the wrap of NYX_HIP_GT_LONGITUDE: a negative angle that + 360 rounds to 360 is 0
                const double deg = atan2(sh.rho_e, -sh.rho_s) * AER_DEG;
                const double w = deg < 0.0 ? deg + 360.0 : deg;
                sh.az_deg = w >= 360.0 ? 0.0 : w;
            }
            if (a.need & AER_NEED_RANGE_RATE) sh.range_rate = (rx * yf[3] + ry * yf[4] + rz * yf[5]) / sh.range;
#pragma unroll 1   // (one copy of the parameter code; p and param[p] are scalars)
            for (int p = 0; p < a.q.n_params; ++p) {
                const double val = aer_value(a.q.param[p], sh);
                if (mine) a.values[(((int64_t)s * a.q.n_params + p) * a.capacity + q) * a.n + i] = ok ? val : qnan;
            }
        }
    }
    // the rest of the tile lies beyond the series
    if (live)
        for (int64_t q = q_end > q0 ? q_end : q0; q < q_hi; ++q)
            for (int64_t r = 0; r < rows; ++r) a.values[(r * a.capacity + q) * a.n + i] = qnan;
}

// The series of a trajectory ENDS at its first failing sample (traj_it.rs:39-61): what later chunks stored after it is
// blanked.  Trajectories without a failing sample (all of them, normally) have nothing to do here.
__global__ __launch_bounds__(256) void nyxaer_seal_kernel(AerArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    int64_t lo, count;
    aer_series(a, make_view(a.src, a.n, i), lo, count);
    const int64_t top = count < a.capacity ? count : a.capacity;
    const int64_t rows = (int64_t)a.q.n_stations * a.q.n_params;
    const double qnan = __builtin_nan("");
    for (int64_t q = a.len[i]; q < top; ++q)
        for (int64_t r = 0; r < rows; ++r) a.values[(r * a.capacity + q) * a.n + i] = qnan;
}

extern "C" hipError_t nyx_launch_traj_aer(const AerArgs *args, hipStream_t stream) {
    AerArgs a = *args;
    if (a.n <= 0 || a.capacity <= 0) return hipSuccess;
    a.need = 0;
    for (int p = 0; p < a.q.n_params; ++p) a.need |= aer_param_needs(a.q.param[p]);
    aer_station_consts(a.q, a.st);
    const dim3 per_traj((unsigned)((a.n + 255) / 256));
    hipLaunchKernelGGL(nyxaer_init_kernel, per_traj, dim3(256), 0, stream, a);
    // one wave per 64 trajectories x a tile of AER_TILE consecutive samples; a launch covers kMaxChunks tiles (series_host.h)
    for (a.sample0 = 0; a.sample0 < a.capacity; a.sample0 += kMaxChunks * AER_TILE) {
        const int64_t left = a.capacity - a.sample0, tiles = (left + AER_TILE - 1) / AER_TILE;
        const dim3 grid((unsigned)((a.n + LANES - 1) / LANES), (unsigned)(tiles < kMaxChunks ? tiles : kMaxChunks));
        hipLaunchKernelGGL(nyxaer_values_kernel, grid, dim3(LANES), 0, stream, a);
    }
    hipLaunchKernelGGL(nyxaer_seal_kernel, per_traj, dim3(256), 0, stream, a);
    return hipGetLastError();
}
