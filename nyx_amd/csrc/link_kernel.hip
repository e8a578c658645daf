// link_kernel.hip — the link report on the MI355X (gfx950): resample every run of a batch AND a transmitter trajectory over the overlap
// of their spans (the span and series rules of ric_kernel.hip), evaluate the ephemerides OF THE CONTEXT at the sample's epoch (as
// eclipse_kernel.hip) and write ONLY the requested values of the link between the two: the range, the range rate, the reference's
// Doppler, the unit line of sight, and whether a body blocks the line - Vallado's SIGHT test per body, with the clearance of the line
// over its limb (include/nyx_hip_link.h).  What `InterlinkTxSpacecraft::measure_instantaneous` (od/interlink/trk_device.rs) forms for
// one pair.  The seventh sibling of report_kernel.hip.
//
// Mapping: lane <-> run; a workgroup is ONE wave that owns 64 runs x a tile of LNK_TILE consecutive samples (grid.y walks the tiles),
// so the dense output is read and values[(p * capacity + k) * n + i] is written fully coalesced.  With one transmitter for the whole
// ensemble (n_ref = 1) every lane reads the same reference words: one cache line per wave-load.
//
// TWO PASSES, for the reason aer_kernel.hip documents (profiles/HISTORY.md, "Station views"): nothing of the second pass may be alive
// across `traj_at`.  Pass 1 interpolates the run, THEN the transmitter - ONE rolled loop of two trips around the `traj_at` of
// traj_dev.h, as nyxric_diff_kernel, so there is one copy of HRMINT in the code object and the divided-difference tables of the two
// interpolations are never live together - and parks both states in LDS: twelve doubles per sample, so a tile of 4 samples is the
// siblings' 24 KiB (4 x 12 x 64 lanes x 8 B).  Pass 2 walks the parked states (link_dev.h): every DISTINCT segment of the chains in
// use evaluated once per sample, per lane, at the lane's own sample epoch, position only, and parked in LDS too (12 KiB, a column per
// lane, written and read by that lane alone, no barrier) because the chains index the segments with a scalar that is not a
// compile-time constant; the chains summed in chain order; the SIGHT test per body; the parameters.  With the default body - the
// context's centre, an empty chain - no segment is evaluated at all.  No loop encloses both passes.
//
// `need`, `body_mask`, `param[p]`, `param_body[p]` and the chain tables are kernel arguments - the same for every lane - so the loops
// over segments, bodies and parameters are rolled with scalar branches.  No atomics beyond the family's atomicMin on len.  Bound: FP64
// VALU, by HRMINT's ~1 800 divisions per interpolation, two per sample; the link itself is a few dozen operations.  The formulas are
// restated on the host by nyx_amd/links.py, which is what this kernel is tested against; compiled with -ffp-contract=off.

#include <hip/hip_runtime.h>

#include "../../include/nyx_hip_link.h"
#include "link_args.h"
#include "link_dev.h"
#include "series_host.h"   // kMaxChunks
#include "traj_dev.h"

namespace {

constexpr int LNK_TILE = 4;   // samples a workgroup interpolates (twice each), parks and then evaluates

// lo_i and the count of the inclusive series of run i against its transmitter (ric_series of ric_kernel.hip)
DEVFN void lnk_series(const LnkArgs &a, const View &v, const View &vr, int64_t &lo, int64_t &count) {
    lo = 0;
    count = 0;
    if (v.len <= 0 || vr.len <= 0) return;
    const int64_t first = v.epoch[v.at(0)], last = v.epoch[v.at(v.len - 1)];
    const int64_t rfirst = vr.epoch[vr.at(0)], rlast = vr.epoch[vr.at(vr.len - 1)];
    int64_t start = first > rfirst ? first : rfirst;
    int64_t hi = last < rlast ? last : rlast;
    if (a.q.has_window) {
        start = a.q.start_ns > start ? a.q.start_ns : start;
        hi = a.q.end_ns < hi ? a.q.end_ns : hi;
    }
    if (hi >= start) {
        lo = start;
        count = (hi - start) / a.q.step_ns + 1;
    }
}

DEVFN void lnk_views(const LnkArgs &a, int64_t i, View &v, View &vr) {
    v = make_view(a.src, a.n, i);
    vr = make_view(a.ref, a.n_ref, a.n_ref == 1 ? 0 : i);
}

}  // namespace

// len[i] = the length of the inclusive series (the evaluation kernel lowers it to the first failing sample), epoch0[i] = lo_i
__global__ __launch_bounds__(256) void nyxlnk_init_kernel(LnkArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    View v, vr;
    lnk_views(a, i, v, vr);
    int64_t lo, count;
    lnk_series(a, v, vr, lo, count);
    a.len[i] = count > INT32_MAX ? INT32_MAX : (int32_t)count;
    if (a.epoch0) a.epoch0[i] = lo;
}

// Every slot (p, k < capacity, i) of the tile is written here: the values of a sample at which BOTH trajectories were interpolated
// AND whose epoch lies inside every segment in use, NaN otherwise (a sample that failed, or a slot beyond the series).
__global__ __launch_bounds__(LANES) void nyxlnk_values_kernel(LnkArgs a) {
    __shared__ double parked[LNK_TILE][12][LANES];     // 24 KiB: the interpolated states of the tile, the run's six then the transmitter's
    __shared__ double segpos[ECL_MAX_USEG][3][LANES];  // 12 KiB: the distinct segments' vectors of the sample being evaluated
    const int lane = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * LANES + lane;
    const bool live = i < a.n;
    const int64_t ii = live ? i : a.n - 1;  // idle lanes shadow a valid run and store nothing
    View v, vr;
    lnk_views(a, ii, v, vr);
    int64_t lo, count;
    lnk_series(a, v, vr, lo, count);
    const int64_t q0 = a.sample0 + (int64_t)blockIdx.y * LNK_TILE;
    const int64_t q_hi = q0 + LNK_TILE < a.capacity ? q0 + LNK_TILE : a.capacity;
    const int64_t q_end = count < q_hi ? count : q_hi;  // the samples of THIS run in the tile: [q0, q_end)
    const double qnan = __builtin_nan("");
    uint32_t ok_bits = 0;   // bit t: at sample q0 + t of this lane both trajectories were interpolated
#pragma unroll 1
    for (int t = 0; t < LNK_TILE && __any(q0 + t < q_end); ++t) {
        // lanes past the end of their series ride along on their first epoch (the wave runs one instruction stream)
        const int64_t q = q0 + t;
        const bool mine = live && q < q_end;
        const int64_t epoch = lo + (q < q_end ? q : 0) * a.q.step_ns;
        bool ok = true;
#pragma unroll 1   // (ONE copy of the interpolation, run then transmitter: their tables are never live together)
        for (int w = 0; w < 2; ++w) {
            double s6[6];
            ok = (traj_at(w ? a.ref : a.src, w ? vr : v, epoch, s6) == NYX_HIP_INTERP_OK) && ok;
#pragma unroll
            for (int c = 0; c < 6; ++c) parked[t][w * 6 + c][lane] = s6[c];
        }
        if (mine && !ok) atomicMin(&a.len[i], (int32_t)q);
        ok_bits |= (ok ? 1u : 0u) << t;
    }
#pragma unroll 1
    for (int t = 0; t < LNK_TILE && __any(q0 + t < q_end); ++t) {
        const int64_t q = q0 + t;
        const bool mine = live && q < q_end;
        const int64_t epoch = lo + (q < q_end ? q : 0) * a.q.step_ns;
        // every distinct segment once, at this lane's epoch (none when no body has a chain)
        const int st = lnk_segments(a, ns_to_seconds(epoch), &segpos[0][0][lane], 3 * LANES, LANES);
        const bool interp = (ok_bits >> t) & 1u;
        const bool ok = interp && st == NYX_HIP_OK;
        if (mine && interp && st != NYX_HIP_OK) atomicMin(&a.len[i], (int32_t)q);   // outside the ephemerides: the series ends here
        double rx[6], tx[6];
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            rx[c] = parked[t][c][lane];
            tx[c] = parked[t][6 + c][lane];
        }
        lnk_sample(a, rx, tx, &segpos[0][0][lane], 3 * LANES, LANES, [&](int p, double val) {
            if (mine) a.values[((int64_t)p * a.capacity + q) * a.n + i] = ok ? val : qnan;
        });
    }
    // the rest of the tile lies beyond the series
    if (live)
        for (int64_t q = q_end > q0 ? q_end : q0; q < q_hi; ++q)
            for (int64_t p = 0; p < a.q.n_params; ++p) a.values[(p * a.capacity + q) * a.n + i] = qnan;
}

// The series of a run ENDS at its first failing sample (traj_it.rs:39-61): what later tiles stored after it is blanked.  Runs
// without a failing sample (all of them, normally) have nothing to do here.
__global__ __launch_bounds__(256) void nyxlnk_seal_kernel(LnkArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    View v, vr;
    lnk_views(a, i, v, vr);
    int64_t lo, count;
    lnk_series(a, v, vr, lo, count);
    const int64_t top = count < a.capacity ? count : a.capacity;
    const double qnan = __builtin_nan("");
    for (int64_t q = a.len[i]; q < top; ++q)
        for (int64_t p = 0; p < a.q.n_params; ++p) a.values[(p * a.capacity + q) * a.n + i] = qnan;
}

extern "C" hipError_t nyx_launch_traj_link(const LnkArgs *args, const DevSeg *ctx_seg, hipStream_t stream) {
    LnkArgs a = *args;
    if (a.n <= 0 || a.capacity <= 0) return hipSuccess;
    lnk_needs(a);
    if (!lnk_reduce_chains(a, ctx_seg)) return hipErrorInvalidValue;
    const dim3 per_run((unsigned)((a.n + 255) / 256));
    hipLaunchKernelGGL(nyxlnk_init_kernel, per_run, dim3(256), 0, stream, a);
    // one wave per 64 runs x a tile of LNK_TILE consecutive samples; a launch covers kMaxChunks tiles (series_host.h)
    for (a.sample0 = 0; a.sample0 < a.capacity; a.sample0 += kMaxChunks * LNK_TILE) {
        const int64_t left = a.capacity - a.sample0, tiles = (left + LNK_TILE - 1) / LNK_TILE;
        const dim3 grid((unsigned)((a.n + LANES - 1) / LANES), (unsigned)(tiles < kMaxChunks ? tiles : kMaxChunks));
        hipLaunchKernelGGL(nyxlnk_values_kernel, grid, dim3(LANES), 0, stream, a);
    }
    hipLaunchKernelGGL(nyxlnk_seal_kernel, per_run, dim3(256), 0, stream, a);
    return hipGetLastError();
}
