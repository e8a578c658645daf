// frame_kernel.hip — the encounter report on the MI355X (gfx950): resample every trajectory of a batch (`Traj::every` /
// `Traj::every_between`, md/trajectory/traj.rs:148-162), evaluate the state of ANOTHER CENTRE from the ephemerides of the context at
// the sample's epoch, translate the interpolated state to it (`Traj::to_frame`, md/trajectory/sc_traj.rs:88-129, between two frames of
// one orientation) and write ONLY the requested values about that centre: the nineteen parameters of nyx_hip_traj_values with the
// target's mu, C3, the B-plane (cosmic/bplane.rs) and the hyperbolic excess speed (include/nyx_hip_frame.h).  A sibling of
// eclipse_kernel.hip, whose header comment explains the structure kept here.
//
// Mapping: lane <-> trajectory; a workgroup is ONE wave that owns 64 trajectories x a tile of FRM_TILE consecutive samples (grid.y
// walks the tiles), so the dense output is read and values[(p * capacity + k) * n + i] is written fully coalesced.  The
// interpolation is `traj_at` of traj_dev.h, the code nyx_traj_eval_kernel runs.
//
// TWO PASSES, for the reason eclipse_kernel.hip and aer_kernel.hip document: nothing of the second pass may be alive across
// `traj_at`.  Pass 1 interpolates the tile and parks the SIX components in LDS - 8 samples x 6 x 64 lanes x 8 B = 24 KiB, the figure
// the siblings use.  Pass 2 walks the parked states: every DISTINCT segment of the target's chain is evaluated once per sample, per
// lane, at the lane's own sample epoch (frame_dev.h: the Clenshaw recurrence, with the companion derivative only when a requested
// parameter needs the velocity; the segment rows are kernel arguments, scalar loads) and its position and velocity parked in LDS too
// (4 x 6 x 64 x 8 B = 12 KiB, a column per lane, written and read by that lane alone, no barrier) because the chain indexes the
// segments with a scalar that is not a compile-time constant; then the chain is summed in chain order (the additions of the oracle's
// frame_shift), subtracted from the parked state, the shared intermediates that `need` names evaluated once, and the parameters
// written.  No loop encloses both passes.
//
// `need`, `param[p]` and the chain are kernel arguments - the same for every lane - so the loops over segments and parameters are
// rolled with scalar branches.  No atomics beyond the family's atomicMin on len.  The formulas are restated on the host by
// nyx_amd/frames.py, which is what this kernel is tested against; compiled with -ffp-contract=off.

#include <hip/hip_runtime.h>

#include "../../include/nyx_hip_frame.h"
#include "frame_args.h"
#include "frame_dev.h"
#include "series_host.h"   // kMaxChunks
#include "traj_dev.h"

namespace {

constexpr int FRM_TILE = 8;   // samples a workgroup interpolates, parks and then evaluates

// The first and the count of the inclusive series of one trajectory (TimeSeries::inclusive(lo, hi, step))
DEVFN void frm_series(const FrmArgs &a, const View &v, int64_t &lo, int64_t &count) {
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

}  // namespace

// len[i] = the length of the inclusive series (the evaluation kernel lowers it to the first failing sample)
__global__ __launch_bounds__(256) void nyxfrm_init_kernel(FrmArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    int64_t lo, count;
    frm_series(a, make_view(a.src, a.n, i), lo, count);
    a.len[i] = count > INT32_MAX ? INT32_MAX : (int32_t)count;
}

// Every slot (p, k < capacity, i) of the tile is written here: the values of a sample that was interpolated AND whose epoch lies
// inside every segment of the chain, NaN otherwise (a sample that failed, or a slot beyond the series).
__global__ __launch_bounds__(LANES) void nyxfrm_values_kernel(FrmArgs a) {
    __shared__ double parked[FRM_TILE][6][LANES];     // 24 KiB: the interpolated states of the tile
    __shared__ double segpv[FRM_MAX_USEG][6][LANES];  // 12 KiB: the distinct segments' states of the sample being evaluated
    const int lane = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * LANES + lane;
    const bool live = i < a.n;
    const int64_t ii = live ? i : a.n - 1;  // idle lanes shadow a valid trajectory and store nothing
    const View v = make_view(a.src, a.n, ii);
    int64_t lo, count;
    frm_series(a, v, lo, count);
    const int64_t q0 = a.sample0 + (int64_t)blockIdx.y * FRM_TILE;
    const int64_t q_hi = q0 + FRM_TILE < a.capacity ? q0 + FRM_TILE : a.capacity;
    const int64_t q_end = count < q_hi ? count : q_hi;  // the samples of THIS trajectory in the tile: [q0, q_end)
    const double qnan = __builtin_nan("");
    uint32_t ok_bits = 0;   // bit t: sample q0 + t of this lane was interpolated
#pragma unroll 1
    for (int t = 0; t < FRM_TILE && __any(q0 + t < q_end); ++t) {
        // lanes past the end of their series ride along on their first epoch (the wave runs one instruction stream)
        const int64_t q = q0 + t;
        const bool mine = live && q < q_end;
        const int64_t epoch = lo + (q < q_end ? q : 0) * a.q.step_ns;
        double s6[6];
        const bool ok = traj_at(a.src, v, epoch, s6) == NYX_HIP_INTERP_OK;
        if (mine && !ok) atomicMin(&a.len[i], (int32_t)q);
#pragma unroll
        for (int c = 0; c < 6; ++c) parked[t][c][lane] = s6[c];
        ok_bits |= (ok ? 1u : 0u) << t;
    }
    const bool with_v = (a.need & FRM_NEED_VELOCITY) != 0;
#pragma unroll 1
    for (int t = 0; t < FRM_TILE && __any(q0 + t < q_end); ++t) {
        const int64_t q = q0 + t;
        const bool mine = live && q < q_end;
        const int64_t epoch = lo + (q < q_end ? q : 0) * a.q.step_ns;
        const double et = ns_to_seconds(epoch);
        // every distinct segment once, at this lane's epoch
        int st = NYX_HIP_OK;
#pragma unroll 1
        for (int u = 0; u < a.n_useg; ++u) {
            double p[3], pv[3] = {0.0, 0.0, 0.0};
            const int s1 = frm_cheby_pv(a.seg[u], a.records, et, with_v, p, pv);
            if (s1) st = s1;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                segpv[u][c][lane] = p[c];
                segpv[u][3 + c][lane] = pv[c];
            }
        }
        const bool interp = (ok_bits >> t) & 1u;
        const bool ok = interp && st == NYX_HIP_OK;
        if (mine && interp && st != NYX_HIP_OK) atomicMin(&a.len[i], (int32_t)q);   // outside the ephemerides: the series ends here
        // the target: its chain in chain order, then rv' = rv - body
        double y[6];
        {
            double b[6];
            chain_sum<6>(a.chain, &segpv[0][0][lane], 6 * LANES, LANES, b);
            // (an empty chain subtracts +0: the identity, bit for bit - a signed zero of the state included)
#pragma unroll
            for (int c = 0; c < 6; ++c) y[c] = parked[t][c][lane] - b[c];
        }
        FrmShared sh;
        if (a.need & FRM_NEED_ELEMENTS) frm_shared(a.need, a.q.mu_km3_s2, y, sh);
#pragma unroll 1   // (one copy of the parameter code; p and param[p] are scalars)
        for (int p = 0; p < a.q.n_params; ++p) {
            const double val = frm_param(a.q.param[p], a.q.mu_km3_s2, y, sh);
            if (mine) a.values[((int64_t)p * a.capacity + q) * a.n + i] = ok ? val : qnan;
        }
    }
    // the rest of the tile lies beyond the series
    if (live)
        for (int64_t q = q_end > q0 ? q_end : q0; q < q_hi; ++q)
            for (int64_t p = 0; p < a.q.n_params; ++p) a.values[(p * a.capacity + q) * a.n + i] = qnan;
}

// The series of a trajectory ENDS at its first failing sample (traj_it.rs:39-61): what later tiles stored after it is
// blanked.  Trajectories without a failing sample (all of them, normally) have nothing to do here.
__global__ __launch_bounds__(256) void nyxfrm_seal_kernel(FrmArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    int64_t lo, count;
    frm_series(a, make_view(a.src, a.n, i), lo, count);
    const int64_t top = count < a.capacity ? count : a.capacity;
    const double qnan = __builtin_nan("");
    for (int64_t q = a.len[i]; q < top; ++q)
        for (int64_t p = 0; p < a.q.n_params; ++p) a.values[(p * a.capacity + q) * a.n + i] = qnan;
}

extern "C" hipError_t nyx_launch_traj_frame_values(const FrmArgs *args, const DevSeg *ctx_seg, hipStream_t stream) {
    FrmArgs a = *args;
    if (a.n <= 0 || a.capacity <= 0) return hipSuccess;
    frm_needs(a);
    frm_reduce_chain(a, ctx_seg);
    const dim3 per_traj((unsigned)((a.n + 255) / 256));
    hipLaunchKernelGGL(nyxfrm_init_kernel, per_traj, dim3(256), 0, stream, a);
    // one wave per 64 trajectories x a tile of FRM_TILE consecutive samples; a launch covers kMaxChunks tiles (series_host.h)
    for (a.sample0 = 0; a.sample0 < a.capacity; a.sample0 += kMaxChunks * FRM_TILE) {
        const int64_t left = a.capacity - a.sample0, tiles = (left + FRM_TILE - 1) / FRM_TILE;
        const dim3 grid((unsigned)((a.n + LANES - 1) / LANES), (unsigned)(tiles < kMaxChunks ? tiles : kMaxChunks));
        hipLaunchKernelGGL(nyxfrm_values_kernel, grid, dim3(LANES), 0, stream, a);
    }
    hipLaunchKernelGGL(nyxfrm_seal_kernel, per_traj, dim3(256), 0, stream, a);
    return hipGetLastError();
}
