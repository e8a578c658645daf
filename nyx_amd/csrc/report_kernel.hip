// report_kernel.hip — fused device reports on the MI355X (gfx950): resample every trajectory of a batch
// (`Traj::every` / `Traj::every_between`, md/trajectory/traj.rs:148-162), evaluate up to eight state parameters from the
// interpolated state and write ONLY the values (include/nyx_hip_reports.h).
//
// Mapping: as traj_kernel.hip - lane <-> trajectory, a workgroup is ONE wave that owns 64 trajectories x a chunk of
// consecutive samples (grid.y walks the chunks), so the dense output is read and values[(p * capacity + k) * n + i] is
// written fully coalesced.  The interpolation is `traj_at` of traj_dev.h, the code nyx_traj_eval_kernel runs: the six numbers
// a parameter is evaluated from are bit-identical to what nyx_hip_traj_every returns for that epoch.
//
// Bound: FP64 VALU, by HRMINT's ~1 800 divisions per sample (traj_kernel.hip).  The parameter block adds a few dozen
// FP64 operations, at most three square roots and one atan2 / acos / pow per requested parameter; it starts after the
// divided-difference tables are dead, so it does not add to the register peak of the interpolation.  Which shared
// intermediates (|r|, |v|, h, energy, a, e-vector) are built is decided by `need`, a kernel argument: scalar branches,
// the same for every lane.
//
// The formulas restate nyx_amd/params.py:state_value expression for expression (operand order of numpy's norm, sum and
// cross along an axis of three: ((a0 + a1) + a2); np.mod; clip before acos), compiled with -ffp-contract=off, because
// that host function is what the users of the list reports get today and what this kernel is tested against.

#include <hip/hip_runtime.h>

#include "../../include/nyx_hip_reports.h"
#include "report_args.h"
#include "series_host.h"   // series_chunks
#include "traj_dev.h"

namespace {

constexpr double REP_DEG = 180.0 / 3.14159265358979323846;  // np.degrees: x * (180 / pi)

// `_wrap360` of params.py: np.mod(a, 360) (the remainder takes the divisor's sign, a zero remainder is +0), then the
// `a < 0 -> a + 360` select, which np.mod has already made a no-op
DEVFN double rep_wrap360(double a) {
    double m = fmod(a, 360.0);
    if (m != 0.0) {
        if (m < 0.0) m = m + 360.0;
    } else {
        m = 0.0;
    }
    return m < 0.0 ? m + 360.0 : m;
}

// The first and the count of the inclusive series of one trajectory (TimeSeries::inclusive(lo, hi, step))
DEVFN void rep_series(const ValuesArgs &a, const View &v, int64_t &lo, int64_t &count) {
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

struct RepShared {  // what several parameters of one sample have in common
    double rmag, vmag, h0, h1, h2, hmag, energy, sma, e0, e1, e2, ecc;
};

DEVFN void rep_shared(int32_t need, double mu, const double y[6], RepShared &s) {
    if (need & REP_NEED_R) s.rmag = sqrt((y[0] * y[0] + y[1] * y[1]) + y[2] * y[2]);
    if (need & REP_NEED_V) s.vmag = sqrt((y[3] * y[3] + y[4] * y[4]) + y[5] * y[5]);
    if (need & REP_NEED_H) {
        s.h0 = y[1] * y[5] - y[2] * y[4];
        s.h1 = y[2] * y[3] - y[0] * y[5];
        s.h2 = y[0] * y[4] - y[1] * y[3];
        s.hmag = sqrt((s.h0 * s.h0 + s.h1 * s.h1) + s.h2 * s.h2);
    }
    if (need & REP_NEED_ENERGY) s.energy = 0.5 * s.vmag * s.vmag - mu / s.rmag;
    if (need & REP_NEED_SMA) s.sma = -mu / (2.0 * s.energy);
    if (need & REP_NEED_EVEC) {
        const double k = s.vmag * s.vmag - mu / s.rmag;
        const double rv = (y[0] * y[3] + y[1] * y[4]) + y[2] * y[5];
        s.e0 = (k * y[0] - rv * y[3]) / mu;
        s.e1 = (k * y[1] - rv * y[4]) / mu;
        s.e2 = (k * y[2] - rv * y[5]) / mu;
        s.ecc = sqrt((s.e0 * s.e0 + s.e1 * s.e1) + s.e2 * s.e2);
    }
}

// `param` is the same for every lane (a kernel argument): the chain below is a scalar branch
DEVFN double rep_value(int32_t param, double mu, const double y[6], const RepShared &s) {
    switch (param) {
    case NYX_HIP_SP_X: return y[0];
    case NYX_HIP_SP_Y: return y[1];
    case NYX_HIP_SP_Z: return y[2];
    case NYX_HIP_SP_VX: return y[3];
    case NYX_HIP_SP_VY: return y[4];
    case NYX_HIP_SP_VZ: return y[5];
    case NYX_HIP_SP_RMAG: return s.rmag;
    case NYX_HIP_SP_VMAG: return s.vmag;
    case NYX_HIP_SP_HMAG: return s.hmag;
    case NYX_HIP_SP_ENERGY: return s.energy;
    case NYX_HIP_SP_SEMI_MAJOR_AXIS: return s.sma;
    case NYX_HIP_SP_ECCENTRICITY: return s.ecc;
    case NYX_HIP_SP_APOAPSIS_RADIUS: return s.sma * (1.0 + s.ecc);
    case NYX_HIP_SP_PERIAPSIS_RADIUS: return s.sma * (1.0 - s.ecc);
    case NYX_HIP_SP_PERIOD: return 6.283185307179586 * sqrt(pow(s.sma, 3.0) / mu);
    case NYX_HIP_SP_INCLINATION: {
        const double c = s.h2 / s.hmag;
        return acos(c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c)) * REP_DEG;  // (a NaN passes the clip, as in np.clip)
    }
    case NYX_HIP_SP_RAAN: return rep_wrap360(atan2(s.h0, -s.h1) * REP_DEG);  // node n = z x h = (-h1, h0, 0)
    case NYX_HIP_SP_AOP: {
        // angle from the node to the eccentricity vector, in the orbit plane around h; n2 = 0 enters as in np.cross / np.sum
        const double n0 = -s.h1, n1 = s.h0, n2 = 0.0;
        const double cosw = (n0 * s.e0 + n1 * s.e1) + n2 * s.e2;
        const double c0 = n1 * s.e2 - n2 * s.e1, c1 = n2 * s.e0 - n0 * s.e2, c2 = n0 * s.e1 - n1 * s.e0;
        const double sinw = ((c0 * s.h0 + c1 * s.h1) + c2 * s.h2) / s.hmag;
        return rep_wrap360(atan2(sinw, cosw) * REP_DEG);
    }
    case NYX_HIP_SP_TRUE_ANOMALY: {
        const double cost = (s.e0 * y[0] + s.e1 * y[1]) + s.e2 * y[2];
        const double c0 = s.e1 * y[2] - s.e2 * y[1], c1 = s.e2 * y[0] - s.e0 * y[2], c2 = s.e0 * y[1] - s.e1 * y[0];
        const double sint = ((c0 * s.h0 + c1 * s.h1) + c2 * s.h2) / s.hmag;
        return rep_wrap360(atan2(sint, cost) * REP_DEG);
    }
    default: return __builtin_nan("");
    }
}

}  // namespace

// len[i] = the length of the inclusive series (the evaluation kernel lowers it to the first failing sample)
__global__ __launch_bounds__(256) void nyxrep_init_kernel(ValuesArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    int64_t lo, count;
    rep_series(a, make_view(a.src, a.n, i), lo, count);
    a.len[i] = count > INT32_MAX ? INT32_MAX : (int32_t)count;
}

// Every slot (p, k < capacity, i) is written here: the values of an interpolated sample, NaN otherwise (a sample that
// failed, or a slot beyond the series).
__global__ __launch_bounds__(LANES) void nyxrep_values_kernel(ValuesArgs a) {
    const int lane = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * LANES + lane;
    const bool live = i < a.n;
    const int64_t ii = live ? i : a.n - 1;  // idle lanes shadow a valid trajectory and store nothing
    const View v = make_view(a.src, a.n, ii);
    int64_t lo, count;
    rep_series(a, v, lo, count);
    const int64_t q0 = (int64_t)blockIdx.y * a.samples_per_block;
    const int64_t q_hi = q0 + a.samples_per_block < a.capacity ? q0 + a.samples_per_block : a.capacity;
    const int64_t q_end = count < q_hi ? count : q_hi;  // the samples of THIS trajectory in the chunk: [q0, q_end)
    const double qnan = __builtin_nan("");
    for (int64_t q = q0; __any(q < q_end); ++q) {
        // lanes past the end of their series ride along on their first epoch (the wave runs one instruction stream)
        const bool mine = live && q < q_end;
        double s6[6];
        const bool ok = traj_at(a.src, v, lo + (q < q_end ? q : 0) * a.q.step_ns, s6) == NYX_HIP_INTERP_OK;
        RepShared sh;
        rep_shared(a.need, a.q.mu_km3_s2, s6, sh);
        if (mine && !ok) atomicMin(&a.len[i], (int32_t)q);
#pragma unroll 1   // (one copy of the parameter code; p and param[p] are scalars)
        for (int p = 0; p < a.q.n_params; ++p) {
            const double val = rep_value(a.q.param[p], a.q.mu_km3_s2, s6, sh);
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
__global__ __launch_bounds__(256) void nyxrep_seal_kernel(ValuesArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    int64_t lo, count;
    rep_series(a, make_view(a.src, a.n, i), lo, count);
    const int64_t top = count < a.capacity ? count : a.capacity;
    const double qnan = __builtin_nan("");
    for (int64_t q = a.len[i]; q < top; ++q)
        for (int p = 0; p < a.q.n_params; ++p) a.values[((int64_t)p * a.capacity + q) * a.n + i] = qnan;
}

extern "C" hipError_t nyx_launch_traj_values(const ValuesArgs *args, hipStream_t stream) {
    ValuesArgs a = *args;
    if (a.n <= 0 || a.capacity <= 0) return hipSuccess;
    a.need = 0;
    for (int p = 0; p < a.q.n_params; ++p) a.need |= report_param_needs(a.q.param[p]);
    const dim3 per_traj((unsigned)((a.n + 255) / 256));
    hipLaunchKernelGGL(nyxrep_init_kernel, per_traj, dim3(256), 0, stream, a);
    const SeriesChunks chunks = series_chunks(a.capacity);
    a.samples_per_block = chunks.samples_per_block;
    const dim3 grid((unsigned)((a.n + LANES - 1) / LANES), chunks.grid_y);
    hipLaunchKernelGGL(nyxrep_values_kernel, grid, dim3(LANES), 0, stream, a);
    hipLaunchKernelGGL(nyxrep_seal_kernel, per_traj, dim3(256), 0, stream, a);
    return hipGetLastError();
}
