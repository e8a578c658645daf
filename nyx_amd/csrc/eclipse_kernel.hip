// eclipse_kernel.hip — eclipses on the MI355X (gfx950): resample every trajectory of a batch (`Traj::every` / `Traj::every_between`,
// md/trajectory/traj.rs:148-162), evaluate the ephemerides OF THE CONTEXT at the sample's epoch and write ONLY the requested values
// of the shadow model - the percentage of the light source hidden (`ShadowModel::compute`, cosmic/eclipse.rs:69-83), the
// illumination factor, the state, the eclipsing body, and per body the apparent radii, the separation and the margins to the
// penumbra and umbra edges (include/nyx_hip_eclipse.h).  A sibling of aer_kernel.hip, and the first report kernel that reads the
// context's ephemeris records.
//
// Mapping: lane <-> trajectory as in aer_kernel.hip; a workgroup is ONE wave that owns 64 trajectories x a tile of ECL_TILE
// consecutive samples (grid.y walks the tiles), so the dense output is read and values[(p * capacity + k) * n + i] is written fully
// coalesced.  The interpolation is `traj_at` of traj_dev.h, the code nyx_traj_eval_kernel runs.
//
// TWO PASSES, as aer_kernel.hip and for its reason (see there: with the value block inside the sample loop this hipcc parked what is
// alive across `traj_at` in AGPRs through copies under an empty exec mask).  Pass 1 interpolates the tile and parks the inertial
// POSITION in LDS - three components, not six, so the tile is sixteen samples at the station views' 24 KiB.  Pass 2 walks the parked
// positions: every DISTINCT segment of the chains in use is evaluated once per sample, per lane, at the lane's own sample epoch
// (chain_dev.h: the Clenshaw recurrence; the segment rows are kernel arguments, scalar loads) and its vector parked in LDS too
// - a column per lane, written and read by that lane alone, no barrier - because the chains index the segments with a scalar that
// is not a compile-time constant; then the chains are summed in chain order (the additions of the oracle's body_position), then
// the overlap formula per body, then the parameters.  No loop encloses both passes: nothing of the asin / acos constants or the
// Chebyshev window is alive while HRMINT runs.
//
// `need`, `body_mask`, `param[p]`, `param_body[p]` and the chain tables are kernel arguments - the same for every lane - so the
// loops over segments, bodies and parameters are rolled with scalar branches.  No atomics beyond the family's atomicMin on len.
// The formulas are restated on the host by nyx_amd/eclipse.py, which is what this kernel is tested against; compiled with
// -ffp-contract=off.

#include <hip/hip_runtime.h>

#include "../../include/nyx_hip_eclipse.h"
#include "eclipse_args.h"
#include "eclipse_dev.h"
#include "series_host.h"   // kMaxChunks
#include "traj_dev.h"

namespace {

constexpr double ECL_DEG = 180.0 / 3.14159265358979323846;
constexpr int ECL_TILE = 16;   // samples a workgroup interpolates, parks and then evaluates

// The first and the count of the inclusive series of one trajectory (TimeSeries::inclusive(lo, hi, step))
DEVFN void ecl_series(const EclArgs &a, const View &v, int64_t &lo, int64_t &count) {
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

struct EclModel {  // the shadow model of one sample: the body with the largest percentage (strict >, first wins)
    double n_ls, ls_p, best;
    int32_t winner;
};

// `param` is the same for every lane (a kernel argument): the chain below is a scalar branch
DEVFN double ecl_model_value(int32_t param, const EclModel &m) {
    switch (param) {
    case NYX_HIP_ECL_OCCULTATION: return m.best;
    case NYX_HIP_ECL_ILLUMINATION: return fabs(m.best / 100.0 - 1.0);
    case NYX_HIP_ECL_STATE: return m.best == 0.0 ? 0.0 : (m.best == 100.0 ? 2.0 : 1.0);
    case NYX_HIP_ECL_ECLIPSING_BODY: return (double)m.winner;
    case NYX_HIP_ECL_SUN_RANGE: return m.n_ls;
    case NYX_HIP_ECL_SUN_APPARENT_RADIUS: return m.ls_p * ECL_DEG;
    default: return __builtin_nan("");
    }
}
DEVFN double ecl_body_value(int32_t param, double ls_p, const EclDisk &d) {
    switch (param) {
    case NYX_HIP_ECL_BODY_OCCULTATION: return d.pct;
    case NYX_HIP_ECL_BODY_APPARENT_RADIUS: return d.fo_p * ECL_DEG;
    case NYX_HIP_ECL_BODY_SEPARATION: return d.d_p * ECL_DEG;
    case NYX_HIP_ECL_BODY_PENUMBRA_MARGIN: return ((d.d_p - ls_p) - d.fo_p) * ECL_DEG;   // > 0 <=> the formula's "d_p - ls_p > fo_p"
    case NYX_HIP_ECL_BODY_UMBRA_MARGIN: return (d.fo_p - (d.d_p + ls_p)) * ECL_DEG;      // > 0 <=> the formula's "fo_p > d_p + ls_p"
    default: return __builtin_nan("");
    }
}

}  // namespace

// len[i] = the length of the inclusive series (the evaluation kernel lowers it to the first failing sample)
__global__ __launch_bounds__(256) void nyxecl_init_kernel(EclArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    int64_t lo, count;
    ecl_series(a, make_view(a.src, a.n, i), lo, count);
    a.len[i] = count > INT32_MAX ? INT32_MAX : (int32_t)count;
}

// Every slot (p, k < capacity, i) of the tile is written here: the values of a sample that was interpolated AND whose epoch lies
// inside every segment in use, NaN otherwise (a sample that failed, or a slot beyond the series).
__global__ __launch_bounds__(LANES) void nyxecl_values_kernel(EclArgs a) {
    __shared__ double parked[ECL_TILE][3][LANES];      // 24 KiB: the interpolated positions of the tile
    __shared__ double segpos[ECL_MAX_USEG][3][LANES];  // 12 KiB: the distinct segments' vectors of the sample being evaluated
    const int lane = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * LANES + lane;
    const bool live = i < a.n;
    const int64_t ii = live ? i : a.n - 1;  // idle lanes shadow a valid trajectory and store nothing
    const View v = make_view(a.src, a.n, ii);
    int64_t lo, count;
    ecl_series(a, v, lo, count);
    const int64_t q0 = a.sample0 + (int64_t)blockIdx.y * ECL_TILE;
    const int64_t q_hi = q0 + ECL_TILE < a.capacity ? q0 + ECL_TILE : a.capacity;
    const int64_t q_end = count < q_hi ? count : q_hi;  // the samples of THIS trajectory in the tile: [q0, q_end)
    const double qnan = __builtin_nan("");
    uint32_t ok_bits = 0;   // bit t: sample q0 + t of this lane was interpolated
#pragma unroll 1
    for (int t = 0; t < ECL_TILE && __any(q0 + t < q_end); ++t) {
        // lanes past the end of their series ride along on their first epoch (the wave runs one instruction stream)
        const int64_t q = q0 + t;
        const bool mine = live && q < q_end;
        const int64_t epoch = lo + (q < q_end ? q : 0) * a.q.step_ns;
        double s6[6];
        const bool ok = traj_at(a.src, v, epoch, s6) == NYX_HIP_INTERP_OK;
        if (mine && !ok) atomicMin(&a.len[i], (int32_t)q);
#pragma unroll
        for (int c = 0; c < 3; ++c) parked[t][c][lane] = s6[c];
        ok_bits |= (ok ? 1u : 0u) << t;
    }
#pragma unroll 1
    for (int t = 0; t < ECL_TILE && __any(q0 + t < q_end); ++t) {
        const int64_t q = q0 + t;
        const bool mine = live && q < q_end;
        const int64_t epoch = lo + (q < q_end ? q : 0) * a.q.step_ns;
        const double et = ns_to_seconds(epoch);
        const double r[3] = {parked[t][0][lane], parked[t][1][lane], parked[t][2][lane]};
        // every distinct segment once, at this lane's epoch
        int st = NYX_HIP_OK;
#pragma unroll 1
        for (int u = 0; u < a.n_useg; ++u) {
            double p[3];
            const int s1 = frm_cheby_pv(a.seg[u], a.records, et, false, p, nullptr);
            if (s1) st = s1;
            segpos[u][0][lane] = p[0];
            segpos[u][1][lane] = p[1];
            segpos[u][2][lane] = p[2];
        }
        const bool interp = (ok_bits >> t) & 1u;
        const bool ok = interp && st == NYX_HIP_OK;
        if (mine && interp && st != NYX_HIP_OK) atomicMin(&a.len[i], (int32_t)q);   // outside the ephemerides: the series ends here
        // the light source: its chain in chain order
        EclModel m;
        double r_ls[3];
        {
            double b[3];
            chain_sum<3>(a.light, &segpos[0][0][lane], 3 * LANES, LANES, b);
            r_ls[0] = b[0] - r[0]; r_ls[1] = b[1] - r[1]; r_ls[2] = b[2] - r[2];
        }
        m.n_ls = ecl_norm3(r_ls);
        m.ls_p = qnan;
        if (a.need & ECL_NEED_SUN_RADIUS) m.ls_p = ecl_apparent(a.light.radius_km, m.n_ls);
        m.best = 0.0;
        m.winner = -1;
        if (a.need & (ECL_NEED_MODEL | ECL_NEED_BODY)) {
#pragma unroll 1   // (one copy of the body code; b and the chain of body b are scalars)
            for (int b = 0; b < a.q.n_bodies; ++b) {
                if (!(a.need & ECL_NEED_MODEL) && !((a.body_mask >> b) & 1)) continue;
                const EclChain &ch = a.body[b];
                double pb[3];
                chain_sum<3>(ch, &segpos[0][0][lane], 3 * LANES, LANES, pb);
                const double r_eb[3] = {r[0] - pb[0], r[1] - pb[1], r[2] - pb[2]};
                const EclDisk d = ecl_occultation(m.ls_p, m.n_ls, ch.radius_km, r_eb, r_ls);
                if (d.pct > m.best) { m.best = d.pct; m.winner = b; }
                if ((a.body_mask >> b) & 1) {
#pragma unroll 1   // (one copy of the parameter code; p, param[p] and param_body[p] are scalars)
                    for (int p = 0; p < a.q.n_params; ++p) {
                        if (!ecl_param_per_body(a.q.param[p]) || a.q.param_body[p] != b) continue;
                        const double val = ecl_body_value(a.q.param[p], m.ls_p, d);
                        if (mine) a.values[((int64_t)p * a.capacity + q) * a.n + i] = ok ? val : qnan;
                    }
                }
            }
        }
#pragma unroll 1
        for (int p = 0; p < a.q.n_params; ++p) {
            if (ecl_param_per_body(a.q.param[p])) continue;
            const double val = ecl_model_value(a.q.param[p], m);
            if (mine) a.values[((int64_t)p * a.capacity + q) * a.n + i] = ok ? val : qnan;
        }
    }
    // the rest of the tile lies beyond the series
    if (live)
        for (int64_t q = q_end > q0 ? q_end : q0; q < q_hi; ++q)
            for (int64_t p = 0; p < a.q.n_params; ++p) a.values[(p * a.capacity + q) * a.n + i] = qnan;
}

// The series of a trajectory ENDS at its first failing sample (traj_it.rs:39-61): what later chunks stored after it is
// blanked.  Trajectories without a failing sample (all of them, normally) have nothing to do here.
__global__ __launch_bounds__(256) void nyxecl_seal_kernel(EclArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    int64_t lo, count;
    ecl_series(a, make_view(a.src, a.n, i), lo, count);
    const int64_t top = count < a.capacity ? count : a.capacity;
    const double qnan = __builtin_nan("");
    for (int64_t q = a.len[i]; q < top; ++q)
        for (int64_t p = 0; p < a.q.n_params; ++p) a.values[(p * a.capacity + q) * a.n + i] = qnan;
}

extern "C" hipError_t nyx_launch_traj_eclipse(const EclArgs *args, const DevSeg *ctx_seg, hipStream_t stream) {
    EclArgs a = *args;
    if (a.n <= 0 || a.capacity <= 0) return hipSuccess;
    ecl_needs(a);
    if (!ecl_reduce_chains(a, ctx_seg)) return hipErrorInvalidValue;
    const dim3 per_traj((unsigned)((a.n + 255) / 256));
    hipLaunchKernelGGL(nyxecl_init_kernel, per_traj, dim3(256), 0, stream, a);
    // one wave per 64 trajectories x a tile of ECL_TILE consecutive samples; a launch covers kMaxChunks tiles (series_host.h)
    for (a.sample0 = 0; a.sample0 < a.capacity; a.sample0 += kMaxChunks * ECL_TILE) {
        const int64_t left = a.capacity - a.sample0, tiles = (left + ECL_TILE - 1) / ECL_TILE;
        const dim3 grid((unsigned)((a.n + LANES - 1) / LANES), (unsigned)(tiles < kMaxChunks ? tiles : kMaxChunks));
        hipLaunchKernelGGL(nyxecl_values_kernel, grid, dim3(LANES), 0, stream, a);
    }
    hipLaunchKernelGGL(nyxecl_seal_kernel, per_traj, dim3(256), 0, stream, a);
    return hipGetLastError();
}
