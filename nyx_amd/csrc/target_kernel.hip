// target_kernel.hip — the differential-correction targeter on the MI355X (gfx950): the seed and the step of every run of a batch
// (include/nyx_hip_target.h).  What a run does is target_dev.h (restating nyx_amd/targeter.py operation for operation); this file is
// the mapping of runs to lanes and of their states to memory.  Compiled with -ffp-contract=off.
//
// One lane per run, workgroups of TGT_BLOCK = 256 lanes.  Every array is structure-of-arrays: run i of row k of the work block is
// element k n + i of each of its arrays (k = 0 the nominal, k = 1 .. V the perturbed states), what a run keeps between the rounds
// (xi_start, xi, total, prev) is row-major over `cap`: every load and store of a wave is one coalesced row.
//
// SEED (after the launch to the correction epoch): xi_start -> xi, total, prev; the first 1 + V start rows.
//
// STEP (after the in-place propagation of the work block to the achievement epoch), per launch:
//   * lane k < n_chain of a workgroup evaluates segment k of the objective target's chain at the achievement epoch - one epoch for the
//     whole batch - into LDS (Clenshaw with the companion derivative, frm_cheby_pv); ONE barrier; every lane then sums the chain in
//     chain order from zero, as frames.body_state does
//   * a run that is still active reads its 1 + V final rows and their propagation statuses and takes the step of target_dev.h; the
//     Jacobian of the round is parked in the run's own rows of `keep` while the parameters are evaluated and read back for the solve
//     (held in registers beside the parameter code the kernel needed 322 VGPRs, one wave a SIMD; parked 253, two); the run's
//     start state, whose VNC frame is the correction frame, is read inside the step right before the update for the same reason
//   * it then either writes its next 1 + V start rows, or ENDS: status, iteration, correction, errors, the corrected and the achieved
//     state go to the outputs, and the epochs of its work rows are set to the achievement epoch, so that every later propagation
//     launch gives those rows zero duration - a run that has ended stops costing propagation time
//   * a wave adds the population count of its still-active lanes to active[it] with one integer atomic: the 4 bytes the host reads
// No floating-point atomics, no scratch, no inline assembly.
#include <hip/hip_runtime.h>

#include "../../include/nyx_hip_target.h"
#include "hifitime_dev.h"
#include "target_args.h"
#include "target_dev.h"

namespace {

constexpr int TGT_BLOCK = 256;

// rows 6 .. 12 of a state (Cr, Cd, the masses, the areas) from `src` element s to `dst` element d; a row one side lacks is skipped / zero
__device__ __forceinline__ void tgt_copy_tail(const TgtRows &src, int64_t s, const TgtRows &dst, int64_t d) {
#pragma unroll
    for (int c = 6; c < 13; ++c)
        if (dst.f[c]) dst.f[c][d] = src.f[c] ? src.f[c][s] : 0.0;
}

// the 1 + V start rows of run i from xi (`frm`: xi_start)
__device__ __forceinline__ void tgt_write_starts(const TgtArgs &a, int64_t i, const double frm[6], const double xi[6]) {
#pragma unroll 1
    for (int k = 0; k <= a.q.n_vars; ++k) {
        double x[6];
        tgt_start_state(a.q, frm, xi, k, x);
        const int64_t row = (int64_t)k * a.n + i;
        a.work.epoch[row] = a.q.correction_epoch_ns;
#pragma unroll
        for (int c = 0; c < 6; ++c) a.work.f[c][row] = x[c];
        tgt_copy_tail(a.start, i, a.work, row);
    }
}

}  // namespace

__global__ __launch_bounds__(TGT_BLOCK) void nyxtgt_seed_kernel(TgtArgs a) {
    const int64_t i = (int64_t)blockIdx.x * TGT_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    double xs[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) xs[c] = a.start.f[c][i];
    TgtRun run;
    tgt_seed(a.q, xs, run);
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        a.keep[(int64_t)(TGT_XI_START + c) * a.cap + i] = xs[c];
        a.keep[(int64_t)(TGT_XI + c) * a.cap + i] = run.xi[c];
        a.keep[(int64_t)(TGT_TOTAL + c) * a.cap + i] = run.total[c];
    }
    a.keep[(int64_t)TGT_PREV * a.cap + i] = run.prev;
    a.flag[i] = a.start.status[i] != NYX_HIP_OK ? TGT_RUN_LEG_FAILED : TGT_RUN_ACTIVE;
    tgt_write_starts(a, i, xs, run.xi);
}

__global__ __launch_bounds__(TGT_BLOCK) void nyxtgt_step_kernel(TgtArgs a) {
    __shared__ double seg_rv[NYX_HIP_MAX_CHAIN][6];
    __shared__ int seg_st[NYX_HIP_MAX_CHAIN];
    const int tid = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * TGT_BLOCK + tid;
    if (tid < a.chain.n_chain) {
        double r[3], v[3];
        seg_st[tid] = frm_cheby_pv(a.chain.seg[tid], a.records, ns_to_seconds(a.q.achievement_epoch_ns), true, r, v);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            seg_rv[tid][c] = r[c];
            seg_rv[tid][3 + c] = v[c];
        }
    }
    __syncthreads();
    const int flag = i < a.n ? a.flag[i] : TGT_RUN_ENDED;
    bool goes_on = false;
    if (flag != TGT_RUN_ENDED) {
        // the objective target about the context's centre: the signed sum along the chain, in chain order, from zero
        double body[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        bool ephem_bad = false;
#pragma unroll
        for (int k = 0; k < NYX_HIP_MAX_CHAIN; ++k)
            if (k < a.chain.n_chain) {
                ephem_bad = ephem_bad || seg_st[k] != NYX_HIP_OK;
#pragma unroll
                for (int c = 0; c < 6; ++c) body[c] = body[c] + a.chain.sign[k] * seg_rv[k][c];
            }
        TgtRun run;
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            run.xi[c] = a.keep[(int64_t)(TGT_XI + c) * a.cap + i];
            run.total[c] = a.keep[(int64_t)(TGT_TOTAL + c) * a.cap + i];
        }
        run.prev = a.keep[(int64_t)TGT_PREV * a.cap + i];
        const bool translate = a.chain.n_chain > 0;
        const int leg = flag == TGT_RUN_LEG_FAILED ? 1 : 0;
        double err[TGT_MO];
        const int st = tgt_step(a.q, a.need, a.it, ephem_bad, [&](int k, double y[6]) -> int {
            const int64_t row = (int64_t)k * a.n + i;
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                const double w = a.work.f[c][row];
                y[c] = translate ? w - body[c] : w;
            }
            return a.work.status[row] | leg;
        }, a.keep + (int64_t)TGT_PARK * a.cap + i, a.cap, a.keep + (int64_t)TGT_XI_START * a.cap + i, a.cap, run, err);
        goes_on = st == TGT_GOES_ON;
        double xs[6];
#pragma unroll
        for (int c = 0; c < 6; ++c) xs[c] = a.keep[(int64_t)(TGT_XI_START + c) * a.cap + i];
        if (goes_on) {
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                a.keep[(int64_t)(TGT_XI + c) * a.cap + i] = run.xi[c];
                a.keep[(int64_t)(TGT_TOTAL + c) * a.cap + i] = run.total[c];
            }
            a.keep[(int64_t)TGT_PREV * a.cap + i] = run.prev;
            tgt_write_starts(a, i, xs, run.xi);
        } else {
            a.flag[i] = TGT_RUN_ENDED;
            a.o_status[i] = st;
            a.o_iterations[i] = a.it;
#pragma unroll
            for (int j = 0; j < TGT_MV; ++j)
                if (j < a.q.n_vars) a.o_correction[(int64_t)j * a.n + i] = run.total[j];
#pragma unroll
            for (int o = 0; o < TGT_MO; ++o)
                if (o < a.q.n_objs) a.o_errors[(int64_t)o * a.n + i] = err[o];
            double xc[6];
            tgt_corrected(a.q, xs, run.total, xc);
            a.corrected.epoch[i] = a.q.correction_epoch_ns;
            a.achieved.epoch[i] = a.work.epoch[i];
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                a.corrected.f[c][i] = xc[c];
                a.achieved.f[c][i] = a.work.f[c][i];
            }
            tgt_copy_tail(a.start, i, a.corrected, i);
            tgt_copy_tail(a.work, i, a.achieved, i);
#pragma unroll 1
            for (int k = 0; k <= a.q.n_vars; ++k) a.work.epoch[(int64_t)k * a.n + i] = a.q.achievement_epoch_ns;
        }
    }
    const unsigned long long live = __ballot(goes_on);
    if ((tid & 63) == 0 && live != 0ull) atomicAdd(a.active + a.it, (int)__popcll(live));
}

extern "C" hipError_t nyx_launch_target_seed(const TgtArgs *args, hipStream_t stream) {
    const TgtArgs a = *args;
    if (a.n <= 0) return hipSuccess;
    const int64_t blocks = (a.n + TGT_BLOCK - 1) / TGT_BLOCK;
    if (blocks > INT32_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(nyxtgt_seed_kernel, dim3((unsigned)blocks), dim3(TGT_BLOCK), 0, stream, a);
    return hipGetLastError();
}

extern "C" hipError_t nyx_launch_target_step(const TgtArgs *args, hipStream_t stream) {
    TgtArgs a = *args;
    if (a.n <= 0) return hipSuccess;
    a.need = tgt_needs(a.q);
    const int64_t blocks = (a.n + TGT_BLOCK - 1) / TGT_BLOCK;
    if (blocks > INT32_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(nyxtgt_step_kernel, dim3((unsigned)blocks), dim3(TGT_BLOCK), 0, stream, a);
    return hipGetLastError();
}
