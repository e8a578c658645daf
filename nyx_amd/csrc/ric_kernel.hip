// ric_kernel.hip — fused device report on the MI355X (gfx950): the RIC differences of every run of a batch to a reference
// trajectory over time (`Traj::ric_diff_to_parquet`, md/trajectory/traj.rs:407-600: align the spans, resample both,
// `Orbit::ric_difference` of every pair, `smooth_state_diff_in_place`), and the per-sample sums an ensemble's mean and
// covariance envelope are made of (include/nyx_hip_ric.h).  A sibling of report_kernel.hip: same mapping, same machinery.
//
// Mapping: lane <-> run, a workgroup is ONE wave that owns 64 runs x a chunk of consecutive samples (grid.y walks the
// chunks), so the dense output is read and values[(c * capacity + k) * n + i] is written fully coalesced.  With one nominal
// for the whole ensemble (n_ref = 1) every lane reads the same reference words: one cache line per wave-load.
//
// nyxric_diff_kernel interpolates the run, keeps its six numbers, THEN interpolates the reference - one rolled loop of two
// trips around the `traj_at` of traj_dev.h, so there is one copy of HRMINT in the code object and the divided-difference
// tables of the two interpolations are never live together: the register peak is that of nyx_traj_eval_kernel
// (tests/test_ric_budget.py holds it to that kernel's budget).  Both states are bit-identical to what nyx_hip_traj_every
// returns for that epoch.  Bound: FP64 VALU, by HRMINT's ~1 800 divisions per interpolation (traj_kernel.hip), two per
// sample here; the difference itself is ~60 FP64 operations, 7 divisions and 2 square roots.
//
// The difference restates nyx_amd/params.py:ric_difference expression for expression (sums of three as ((a0 + a1) + a2)),
// compiled with -ffp-contract=off: only +, -, x, / and sqrt, all IEEE operations, so the device agrees with that host
// function to the last bit.
//
// nyxric_smooth_kernel (the median filter, lane <-> run, k ascending with a rolling register window) and
// nyxric_moments_kernel (one workgroup per sample, fixed summation order, no atomics) are memory-bound and small:
// 2 x 48 B and 48 B per stored sample against the ~4 000 divisions the sample cost to make.  The moments grid is one
// workgroup of 256 threads per sample whatever n is (each re-reads len[0 .. n), coalesced): sized for ensembles of
// thousands, not tuned for a dozen runs, where most lanes add zeros.
//
// Degenerate frame state: |f_r| = 0 or |h| = 0 (no orbit has either) divides by zero, so that sample's d holds NaN although
// both interpolations succeeded.  Such a sample still counts in len[i] and in the count of the moments, and turns the sums
// of its sample index into NaN.  The filter's compare-and-swap (`b < a`) never moves a NaN, where numpy's sort puts it last
// and the reference panics: for such a run the filtered device values and smooth_ric may differ.  Unspecified, not guarded.

#include <hip/hip_runtime.h>

#include "../../include/nyx_hip_ric.h"
#include "ric_args.h"
#include "series_host.h"   // series_chunks
#include "traj_dev.h"

namespace {

constexpr int RIC_HALF_MAX = NYX_HIP_RIC_MAX_WINDOW / 2;
constexpr int RIC_MOM_THREADS = 256;

// lo_i and the count of the inclusive series of run i against its reference trajectory
DEVFN void ric_series(const RicArgs &a, const View &v, const View &vr, int64_t &lo, int64_t &count) {
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

DEVFN void ric_views(const RicArgs &a, int64_t i, View &v, View &vr) {
    v = make_view(a.src, a.n, i);
    vr = make_view(a.ref, a.n_ref, a.n_ref == 1 ? 0 : i);
}

// params.py:ric_difference; `frame_of` and `transport` are kernel arguments: scalar selects, the same for every lane
DEVFN void ric_difference(const double x[6], const double r[6], int frame_of, int transport, double out[6]) {
    double d[6], f[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        d[c] = x[c] - r[c];
        f[c] = frame_of ? r[c] : x[c];
    }
    const double rmag = sqrt((f[0] * f[0] + f[1] * f[1]) + f[2] * f[2]);
    const double r0 = f[0] / rmag, r1 = f[1] / rmag, r2 = f[2] / rmag;
    const double h0 = f[1] * f[5] - f[2] * f[4];
    const double h1 = f[2] * f[3] - f[0] * f[5];
    const double h2 = f[0] * f[4] - f[1] * f[3];
    const double hmag = sqrt((h0 * h0 + h1 * h1) + h2 * h2);
    const double c0 = h0 / hmag, c1 = h1 / hmag, c2 = h2 / hmag;
    const double i0 = c1 * r2 - c2 * r1, i1 = c2 * r0 - c0 * r2, i2 = c0 * r1 - c1 * r0;
    out[0] = (r0 * d[0] + r1 * d[1]) + r2 * d[2];
    out[1] = (i0 * d[0] + i1 * d[1]) + i2 * d[2];
    out[2] = (c0 * d[0] + c1 * d[1]) + c2 * d[2];
    out[3] = (r0 * d[3] + r1 * d[4]) + r2 * d[5];
    out[4] = (i0 * d[3] + i1 * d[4]) + i2 * d[5];
    out[5] = (c0 * d[3] + c1 * d[4]) + c2 * d[5];
    if (transport) {
        const double w = hmag / (rmag * rmag);
        const double vr = out[3] + w * out[1];
        const double vi = out[4] - w * out[0];
        out[3] = vr;
        out[4] = vi;
    }
}

DEVFN void ric_cswap(double &a, double &b) {
    const bool swap = b < a;
    const double lo = swap ? b : a, hi = swap ? a : b;
    a = lo;
    b = hi;
}

}  // namespace

// len[i] = the length of the inclusive series (the evaluation kernel lowers it to the first failing sample), epoch0[i] = lo_i
__global__ __launch_bounds__(256) void nyxric_init_kernel(RicArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    View v, vr;
    ric_views(a, i, v, vr);
    int64_t lo, count;
    ric_series(a, v, vr, lo, count);
    a.len[i] = count > INT32_MAX ? INT32_MAX : (int32_t)count;
    if (a.epoch0) a.epoch0[i] = lo;
}

// Every slot (c, k < capacity, i) is written here: the difference of an interpolated pair, NaN otherwise (a sample at which
// either trajectory failed, or a slot beyond the series).
__global__ __launch_bounds__(LANES) void nyxric_diff_kernel(RicArgs a) {
    const int lane = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * LANES + lane;
    const bool live = i < a.n;
    const int64_t ii = live ? i : a.n - 1;  // idle lanes shadow a valid run and store nothing
    View v, vr;
    ric_views(a, ii, v, vr);
    int64_t lo, count;
    ric_series(a, v, vr, lo, count);
    const int64_t q0 = (int64_t)blockIdx.y * a.samples_per_block;
    const int64_t q_hi = q0 + a.samples_per_block < a.capacity ? q0 + a.samples_per_block : a.capacity;
    const int64_t q_end = count < q_hi ? count : q_hi;  // the samples of THIS run in the chunk: [q0, q_end)
    const double qnan = __builtin_nan("");
    for (int64_t q = q0; __any(q < q_end); ++q) {
        // lanes past the end of their series ride along on their first epoch (the wave runs one instruction stream)
        const bool mine = live && q < q_end;
        const int64_t epoch = lo + (q < q_end ? q : 0) * a.q.step_ns;
        double run6[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, ref6[6];
        bool ok = true;
#pragma unroll 1   // (ONE copy of the interpolation, run then reference: their tables are never live together)
        for (int t = 0; t < 2; ++t) {
            double s6[6];
            ok = (traj_at(t ? a.ref : a.src, t ? vr : v, epoch, s6) == NYX_HIP_INTERP_OK) && ok;
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                run6[c] = t == 0 ? s6[c] : run6[c];
                ref6[c] = s6[c];
            }
        }
        double d6[6];
        ric_difference(run6, ref6, a.q.frame_of, a.q.transport, d6);
        if (mine && !ok) atomicMin(&a.len[i], (int32_t)q);
        if (mine) {
#pragma unroll
            for (int c = 0; c < 6; ++c) a.values[((int64_t)c * a.capacity + q) * a.n + i] = ok ? d6[c] : qnan;
        }
    }
    // the rest of the chunk lies beyond the series
    if (live)
        for (int64_t q = q_end > q0 ? q_end : q0; q < q_hi; ++q)
            for (int c = 0; c < 6; ++c) a.values[((int64_t)c * a.capacity + q) * a.n + i] = qnan;
}

// The series of a run ENDS at its first failing sample (traj_it.rs:39-61): what later chunks stored after it is blanked.
// Runs without a failing sample (all of them, normally) have nothing to do here.
__global__ __launch_bounds__(256) void nyxric_seal_kernel(RicArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    View v, vr;
    ric_views(a, i, v, vr);
    int64_t lo, count;
    ric_series(a, v, vr, lo, count);
    const int64_t top = count < a.capacity ? count : a.capacity;
    const double qnan = __builtin_nan("");
    for (int64_t q = a.len[i]; q < top; ++q)
        for (int c = 0; c < 6; ++c) a.values[((int64_t)c * a.capacity + q) * a.n + i] = qnan;
}

// `smooth_state_diff_in_place` (md/trajectory/mod.rs:75-125) on the stored samples of every run: lane <-> run, k ascending
// and in place.  W[c][j] holds sample k - 4 + j of component c: the entries left of the centre are the medians already
// stored, the centre and the entries right of it are raw; every step stores one median, shifts the window and loads the
// sample five ahead, so every sample is read once and written once, coalesced across the lanes.  The window of the
// request (3 .. 9) and the ends of the series mask entries out (+inf: sorted last); the median is element count / 2 of
// the sorted window, an odd-even transposition network on nine registers.  A median is a selection: no rounding.
__global__ __launch_bounds__(LANES) void nyxric_smooth_kernel(RicArgs a) {
    const int64_t i = (int64_t)blockIdx.x * LANES + threadIdx.x;
    if (i >= a.n) return;
    const int64_t produced = a.len[i];
    const int64_t K = produced < a.capacity ? produced : a.capacity;
    const int window = a.q.smooth_window, half = window / 2;
    if (K <= window) return;   // (the reference filters only when it has more samples than the window)
    constexpr int NW = 2 * RIC_HALF_MAX + 1;
    const double inf = __builtin_inf();
    double W[6][NW];
#pragma unroll
    for (int c = 0; c < 6; ++c)
#pragma unroll
        for (int j = 0; j < NW; ++j) {
            const int64_t k = j - RIC_HALF_MAX;
            W[c][j] = (k >= 0 && k < K) ? a.values[((int64_t)c * a.capacity + k) * a.n + i] : 0.0;
        }
    for (int64_t k = 0; k < K; ++k) {
        const int64_t start = k - half > 0 ? k - half : 0;
        const int64_t end = k + half + 1 < K ? k + half + 1 : K;
        const int pick = (int)(end - start) / 2;   // 1 .. 4
        const int64_t ahead = k + RIC_HALF_MAX + 1;
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            const double next = ahead < K ? a.values[((int64_t)c * a.capacity + ahead) * a.n + i] : 0.0;
            double t[NW];
#pragma unroll
            for (int j = 0; j < NW; ++j) {
                const int64_t at = k + j - RIC_HALF_MAX;
                t[j] = (at >= start && at < end) ? W[c][j] : inf;
            }
#pragma unroll
            for (int round = 0; round < NW; ++round)
#pragma unroll
                for (int j = round & 1; j + 1 < NW; j += 2) ric_cswap(t[j], t[j + 1]);
            const double med = pick == 1 ? t[1] : (pick == 2 ? t[2] : (pick == 3 ? t[3] : t[4]));
            a.values[((int64_t)c * a.capacity + k) * a.n + i] = med;
            W[c][RIC_HALF_MAX] = med;
#pragma unroll
            for (int j = 0; j + 1 < NW; ++j) W[c][j] = W[c][j + 1];
            W[c][NW - 1] = next;
        }
    }
}

// moments[k * 28 ..]: count, sum d[6] and the upper triangle of sum d d^T over the runs that have sample k.  One workgroup
// per sample: lane-strided walk over the runs (coalesced), butterfly sums inside a wave, the four waves added in index
// order - the order depends on n only, no atomics: bit-reproducible (as moments_kernel.hip).
__global__ __launch_bounds__(RIC_MOM_THREADS) void nyxric_moments_kernel(RicArgs a) {
    __shared__ double red[RIC_MOM_THREADS / 64][NYX_HIP_RIC_MOMENTS];
    const int64_t k = blockIdx.x;
    double acc[NYX_HIP_RIC_MOMENTS];
#pragma unroll
    for (int q = 0; q < NYX_HIP_RIC_MOMENTS; ++q) acc[q] = 0.0;
    for (int64_t i = threadIdx.x; i < a.n; i += RIC_MOM_THREADS) {
        if (k >= a.len[i]) continue;   // (k < capacity by the grid)
        double d[6];
#pragma unroll
        for (int c = 0; c < 6; ++c) d[c] = a.values[((int64_t)c * a.capacity + k) * a.n + i];
        acc[0] += 1.0;
#pragma unroll
        for (int c = 0; c < 6; ++c) acc[1 + c] += d[c];
        int q = 7;
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int c = r; c < 6; ++c) acc[q++] += d[r] * d[c];
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < NYX_HIP_RIC_MOMENTS; ++q) {
        double v = acc[q];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
        if (lane == 0) red[wave][q] = v;
    }
    __syncthreads();
    if (threadIdx.x < NYX_HIP_RIC_MOMENTS) {
        double s = red[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < RIC_MOM_THREADS / 64; ++w) s += red[w][threadIdx.x];
        a.moments[k * NYX_HIP_RIC_MOMENTS + threadIdx.x] = s;
    }
}

extern "C" hipError_t nyx_launch_ric_diff(const RicArgs *args, hipStream_t stream) {
    RicArgs a = *args;
    if (a.n <= 0 || a.capacity <= 0) return hipSuccess;
    const dim3 per_run((unsigned)((a.n + 255) / 256));
    const dim3 per_wave((unsigned)((a.n + LANES - 1) / LANES));
    hipLaunchKernelGGL(nyxric_init_kernel, per_run, dim3(256), 0, stream, a);
    const SeriesChunks chunks = series_chunks(a.capacity);
    a.samples_per_block = chunks.samples_per_block;
    const dim3 grid(per_wave.x, chunks.grid_y);
    hipLaunchKernelGGL(nyxric_diff_kernel, grid, dim3(LANES), 0, stream, a);
    hipLaunchKernelGGL(nyxric_seal_kernel, per_run, dim3(256), 0, stream, a);
    if (a.q.smooth_window >= 3) hipLaunchKernelGGL(nyxric_smooth_kernel, per_wave, dim3(LANES), 0, stream, a);
    if (a.moments) hipLaunchKernelGGL(nyxric_moments_kernel, dim3((unsigned)a.capacity), dim3(RIC_MOM_THREADS), 0, stream, a);
    return hipGetLastError();
}
