// lambert_kernel.hip — Lambert transfers on the MI355X (gfx950): a batch of independent problems and a departure x arrival grid
// (include/nyx_hip_lambert.h).  The solver is lambert_dev.h (Izzo's method, restating nyx_amd/lambert.py operation for operation);
// this file is the mapping of problems to lanes.  Compiled with -ffp-contract=off.
//
// BATCH: one problem per lane.  The inputs are component-major (rv[c * n + i]) and so are the values (values[p * n + i]): every load
// and store of a wave is one coalesced row.
//
// GRID: one launch, no global scratch, no atomics.  A workgroup of eight waves owns a tile of LMB_TD = 8 departures x LMB_TA = 64
// arrivals, the arrival index on the lanes, so that values[(p * n_dep + i) * n_arr + j] is written in coalesced rows.  The tile's
// departure states are evaluated once each by the first eight lanes of wave 0 and, where the arrivals are given by epoch, the tile's
// arrival states once each by the lanes of wave 1 at the same time (Clenshaw with the companion derivative, chain_pv of chain_dev.h, the body's
// chain minus the centre's), and parked in LDS: (8 + 64) x 6 doubles and the status words, under 4 KiB.  After ONE barrier wave w
// solves the cells of departure w of the tile: the lane reads its arrival state from LDS and the departure state as an LDS
// broadcast.  Lanes past the edge of the grid take part in the barrier and store nothing.
//
// The tile shape.  A body state costs up to two chains of up to four segments, each three components of two coupled recurrences of
// about a dozen coefficients: 2 x 4 x 3 x 12 x 6 flops, about 1700 FP64 operations at most and typically (one or two segments per
// chain) 500.  A solve is 2 to 6 Householder steps of about 150 operations and two or three transcendentals each, the initial guess
// (pow, or exp and two logs) and the reconstruction: about 2000.  What a tile pays for the ephemerides is two WAVE passes of a body
// state (the lanes of a wave run together, however few are live) against LMB_TD wave passes of a solve: 2 x 500 / (LMB_TD x 2000),
// 25 % for one row, 6 % for four, 3 % for eight, 1.5 % for sixteen.  Against that stands occupancy.  One row per wave keeps the kernel
// under 120 VGPRs (four waves a SIMD); a wave that LOOPS over several rows was compiled to 256 VGPRs and 18 AGPRs, one wave a SIMD
// (the loop-invariant half of the solver is hoisted and kept), so more rows mean more waves: sixteen rows are a workgroup of 1024
// lanes, the only one its compute unit holds, which then idles through every barrier; eight rows are 512 lanes, two workgroups a
// compute unit, one solving while the other evaluates its states.  A 1024 x 1024 grid gives 2048 workgroups, eight per compute unit.
// With arrivals by TIME OF FLIGHT the arrival epoch differs from cell to cell (departure + tof): nothing of the arrival is shared, each
// lane evaluates its own arrival state, and only the departures are parked.
//
// Divergence.  The Householder loop, the Halley loop of the feasibility edge and the series leave by their own lane's test: a wave
// runs until its last lane has left, the lanes that left earlier masked.  Iteration counts differ by a few steps from lane to lane
// (1 to 3 measured without a revolution, 2 to 6 with one), neighbouring cells of a grid mostly agree.  The Householder loop run to a
// wave-uniform trip count (a vote per step, converged lanes masked by hand) was measured 0.4 to 3 % slower and is not kept
// (profiles/HISTORY.md).
#include <hip/hip_runtime.h>

#include "../../include/nyx_hip_lambert.h"
#include "hifitime_dev.h"
#include "lambert_args.h"
#include "lambert_dev.h"

namespace {

constexpr int LMB_TD = 8;       // departures of a tile: one per wave
constexpr int LMB_TA = 64;      // arrivals of a tile: one per lane
constexpr int LMB_BLOCK = 256;  // lanes of a workgroup of the batch kernel
constexpr int LMB_TILE = LMB_TD * LMB_TA;

}  // namespace

__global__ __launch_bounds__(LMB_BLOCK) void nyxlmb_batch_kernel(LmbBatchArgs a) {
    const int64_t i = (int64_t)blockIdx.x * LMB_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    double rv1[6], rv2[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        rv1[c] = a.rv1[(int64_t)c * a.n + i];
        rv2[c] = a.rv2[(int64_t)c * a.n + i];
    }
    LmbSol s;
    const int st = lmb_solve(rv1, rv2, a.tof_s[i], a.mu, a.q, s);
    a.status[i] = st;
    const double qnan = __builtin_nan("");
#pragma unroll 1   // (one copy of the parameter code; p and param[p] are scalars)
    for (int p = 0; p < a.q.n_params; ++p) a.values[(int64_t)p * a.n + i] = st == NYX_HIP_LMB_OK ? lmb_param(a.q.param[p], s) : qnan;
}

__global__ __launch_bounds__(LMB_TILE) void nyxlmb_grid_kernel(LmbGridArgs a, int64_t tiles_a) {
    __shared__ double dep_rv[LMB_TD][6];
    __shared__ double arr_rv[6][LMB_TA];
    __shared__ int dep_st[LMB_TD], arr_st[LMB_TA];
    const nyx_hip_lambert_grid_query_t &q = a.q;
    const int tid = threadIdx.x, wave = tid / LMB_TA, lane = tid % LMB_TA;
    const int64_t tile_d = (int64_t)blockIdx.x / tiles_a, tile_a = (int64_t)blockIdx.x % tiles_a;
    const int64_t i0 = tile_d * LMB_TD, j = tile_a * LMB_TA + lane;
    // the tile's departure states: the first LMB_TD lanes of wave 0 (lanes past the edge ride along on the last departure)
    if (tid < LMB_TD) {
        const int64_t i = i0 + tid < q.n_dep ? i0 + tid : q.n_dep - 1;
        double rv[6];
        dep_st[tid] = lmb_body_state(a.dep, a.centre, a.records, ns_to_seconds(q.dep0_ns + i * q.dep_step_ns), rv);
#pragma unroll
        for (int c = 0; c < 6; ++c) dep_rv[tid][c] = rv[c];
    }
    // its arrival states where they are shared by the departures: wave 1
    if (wave == 1 && !q.has_tof) {
        const int64_t jj = j < q.n_arr ? j : q.n_arr - 1;
        double rv[6];
        arr_st[lane] = lmb_body_state(a.arr, a.centre, a.records, ns_to_seconds(q.arr0_ns + jj * q.arr_step_ns), rv);
#pragma unroll
        for (int c = 0; c < 6; ++c) arr_rv[c][lane] = rv[c];
    }
    __syncthreads();
    const int64_t i = i0 + wave;   // wave w solves the cells of departure w of the tile
    if (i >= q.n_dep || j >= q.n_arr) return;   // (no barrier below)
    const int64_t dep_ns = q.dep0_ns + i * q.dep_step_ns;
    const int64_t arr_ns = q.has_tof ? dep_ns + (q.tof0_ns + j * q.tof_step_ns) : q.arr0_ns + j * q.arr_step_ns;
    double rv1[6], rv2[6];
    int st2;
    if (q.has_tof) {
        st2 = lmb_body_state(a.arr, a.centre, a.records, ns_to_seconds(arr_ns), rv2);
    } else {
        st2 = arr_st[lane];
#pragma unroll
        for (int c = 0; c < 6; ++c) rv2[c] = arr_rv[c][lane];
    }
#pragma unroll
    for (int c = 0; c < 6; ++c) rv1[c] = dep_rv[wave][c];
    LmbSol s;
    int st;
    if (dep_st[wave] != NYX_HIP_OK || st2 != NYX_HIP_OK) st = NYX_HIP_LMB_EPHEM_RANGE;
    else st = lmb_solve(rv1, rv2, ns_to_seconds(arr_ns - dep_ns), q.mu_km3_s2, q.solve, s);
    a.status[i * q.n_arr + j] = st;
    const double qnan = __builtin_nan("");
#pragma unroll 1
    for (int p = 0; p < q.solve.n_params; ++p)
        a.values[((int64_t)p * q.n_dep + i) * q.n_arr + j] = st == NYX_HIP_LMB_OK ? lmb_param(q.solve.param[p], s) : qnan;
}

extern "C" hipError_t nyx_launch_lambert_batch(const LmbBatchArgs *args, hipStream_t stream) {
    const LmbBatchArgs a = *args;
    if (a.n <= 0) return hipSuccess;
    const int64_t blocks = (a.n + LMB_BLOCK - 1) / LMB_BLOCK;
    if (blocks > INT32_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(nyxlmb_batch_kernel, dim3((unsigned)blocks), dim3(LMB_BLOCK), 0, stream, a);
    return hipGetLastError();
}

// `args` holds the query; the chains are resolved here against the context's segment rows
extern "C" hipError_t nyx_launch_lambert_grid(const LmbGridArgs *args, const DevSeg *ctx_seg, hipStream_t stream) {
    LmbGridArgs a = *args;
    if (a.q.n_dep <= 0 || a.q.n_arr <= 0) return hipSuccess;
    a.dep = resolve_chain(chain_view(a.q.dep), ctx_seg);
    a.arr = resolve_chain(chain_view(a.q.arr), ctx_seg);
    a.centre = resolve_chain(chain_view(a.q.centre), ctx_seg);
    const int64_t tiles_d = (a.q.n_dep + LMB_TD - 1) / LMB_TD, tiles_a = (a.q.n_arr + LMB_TA - 1) / LMB_TA;
    if (tiles_d * tiles_a > INT32_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(nyxlmb_grid_kernel, dim3((unsigned)(tiles_d * tiles_a)), dim3(LMB_TILE), 0, stream, a, tiles_a);
    return hipGetLastError();
}
