// stats_kernel.hip — ensemble statistics of a series report, on the device (include/nyx_hip_stats.h).
//
// One workgroup of STAT_THREADS serves one (row, sample): its n values are contiguous (values[(r * capacity + k) * n + i], coalesced
// loads), `len` and `status` are shared by every workgroup and stay in L2.  Three steps:
//   1  one strided pass forms the key of every slot (stat_key_of: STAT_KEY_OUT for a run that is not held or is NaN) and the integer
//      columns - HELD, COUNT, FINITE, the smallest finite run, the extreme keys and the smallest runs that attain them - with INTEGER
//      LDS atomics, whose result does not depend on their order;
//   2  one strided pass adds d = v - SHIFT and d d in a fixed order that depends on n only: strided lanes, a butterfly inside a wave,
//      the four waves in index order through LDS.  No floating-point atomics;
//   3  per probability an EXACT selection on the 64-bit key: a most-significant-digit-first radix select, eight passes of 8 bits
//      over a 256-bin LDS histogram of integer counters, the bin found by a scan over the 256 threads; the upper neighbour s[lo + 1],
//      needed only when g != 0, costs one more pass (the count of keys <= s[lo] and the smallest key above it).
// The same selection runs over two key sources (template parameter): the keys parked in dynamic LDS by step 1 when n <= STAT_LDS_KEYS
// (10 000 runs: 80 KB of the CU's 160 KiB), or re-formed from the row in global memory on every pass.
// Plain HIP C++, every global store a vector store; every branch around a barrier is uniform over the workgroup.
#include <hip/hip_runtime.h>

#include "stats_args.h"
#include "stats_dev.h"

extern __shared__ unsigned long long nyxstat_keys[];

namespace {

constexpr int kNoRun = 0x7FFFFFFF;

template <bool LDS> __device__ __forceinline__ void stat_block(const StatArgs &a, int64_t rk) {
    __shared__ unsigned int hist[STAT_THREADS];
    __shared__ unsigned int wsum[STAT_THREADS / 64];
    __shared__ double red[STAT_THREADS / 64][2];
    __shared__ unsigned long long s_kmin, s_kmax, s_above;
    __shared__ int s_held, s_count, s_finite, s_first, s_argmin, s_argmax;
    __shared__ unsigned int s_bin, s_rank, s_le;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t n = a.n;
    const int64_t k = rk % a.capacity;
    const double *row = a.values + rk * (int64_t)n;
    double *out = a.stats + rk * (int64_t)(NYX_HIP_STAT_FIXED + a.q.n_probs);
    unsigned long long *keys = nyxstat_keys;
    auto key_at = [&](int32_t i) -> unsigned long long {
        if (LDS) return keys[i];
        return stat_key_of(row[i], stat_held(a.len, a.status, a.capacity, k, i));
    };

    hist[tid] = 0u;
    if (tid == 0) {
        s_kmin = STAT_KEY_OUT; s_kmax = 0ull;
        s_held = s_count = s_finite = 0;
        s_first = s_argmin = s_argmax = kNoRun;
    }
    __syncthreads();

    // ---- 1: keys and integer columns
    {
        int held = 0, count = 0, finite = 0, first = kNoRun, imin = kNoRun, imax = kNoRun;
        unsigned long long kmin = STAT_KEY_OUT, kmax = 0ull;   // (every key of C lies strictly between the two)
        for (int32_t i = tid; i < n; i += STAT_THREADS) {
            const bool h = stat_held(a.len, a.status, a.capacity, k, i);
            const unsigned long long key = stat_key_of(row[i], h);
            if (LDS) keys[i] = key;
            held += h ? 1 : 0;
            if (key != STAT_KEY_OUT) {
                ++count;
                if (stat_key_finite(key)) {
                    ++finite;
                    if (first == kNoRun) first = i;
                }
                if (key < kmin) { kmin = key; imin = i; }
                if (key > kmax) { kmax = key; imax = i; }
            }
        }
        atomicAdd(&s_held, held);
        atomicAdd(&s_count, count);
        atomicAdd(&s_finite, finite);
        atomicMin(&s_first, first);
        atomicMin(&s_kmin, kmin);
        atomicMax(&s_kmax, kmax);
        __syncthreads();
        if (kmin == s_kmin) atomicMin(&s_argmin, imin);
        if (kmax == s_kmax) atomicMin(&s_argmax, imax);
        __syncthreads();
    }
    const int32_t m = s_count;
    const int first = s_first;
    const double shift = first != kNoRun ? row[first] : 0.0;

    // ---- 2: the sums, in a fixed order
    {
        double sum = 0.0, sumsq = 0.0;
        for (int32_t i = tid; i < n; i += STAT_THREADS) {
            const unsigned long long key = key_at(i);
            if (key == STAT_KEY_OUT || !stat_key_finite(key)) continue;
            const double d = stat_unkey(key) - shift;
            sum += d;
            sumsq += d * d;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            sum += __shfl_xor(sum, off, 64);
            sumsq += __shfl_xor(sumsq, off, 64);
        }
        if (lane == 0) { red[wave][0] = sum; red[wave][1] = sumsq; }
        __syncthreads();
        if (tid == 0) {
            double s0 = red[0][0], s1 = red[0][1];
#pragma unroll
            for (int w = 1; w < STAT_THREADS / 64; ++w) { s0 += red[w][0]; s1 += red[w][1]; }
            const double nan = stat_double(STAT_NAN_BITS);
            out[NYX_HIP_STAT_HELD] = (double)s_held;
            out[NYX_HIP_STAT_COUNT] = (double)m;
            out[NYX_HIP_STAT_MIN] = m ? stat_unkey(s_kmin) : nan;
            out[NYX_HIP_STAT_MAX] = m ? stat_unkey(s_kmax) : nan;
            out[NYX_HIP_STAT_ARGMIN] = m ? (double)s_argmin : -1.0;
            out[NYX_HIP_STAT_ARGMAX] = m ? (double)s_argmax : -1.0;
            out[NYX_HIP_STAT_FINITE] = (double)s_finite;
            out[NYX_HIP_STAT_SHIFT] = shift;
            out[NYX_HIP_STAT_SUM] = s0;
            out[NYX_HIP_STAT_SUMSQ] = s1;
        }
    }

    // ---- 3: the quantiles (m, lo and g are the same in every thread: the branches below are uniform)
    for (int j = 0; j < a.q.n_probs; ++j) {
        if (m == 0) {
            if (tid == 0) out[NYX_HIP_STAT_FIXED + j] = stat_double(STAT_NAN_BITS);
            continue;
        }
        int32_t lo;
        const double g = stat_quantile_rank(m, a.q.prob[j], &lo);
        if (tid == 0) { s_le = 0u; s_above = STAT_KEY_OUT; }
        // the key of rank lo among all n keys (those of C come first): digit after digit, from the top
        unsigned long long prefix = 0ull;
        unsigned int rank = (unsigned int)lo;
#pragma unroll 1
        for (int shift_bits = 56; shift_bits >= 0; shift_bits -= 8) {
            for (int32_t i = tid; i < n; i += STAT_THREADS) {
                const unsigned long long key = key_at(i);
                const bool in_prefix = shift_bits == 56 || ((key ^ prefix) >> ((shift_bits + 8) & 63)) == 0ull;
                if (in_prefix) atomicAdd(&hist[(unsigned int)(key >> shift_bits) & 255u], 1u);
            }
            __syncthreads();
            const unsigned int c = hist[tid];
            hist[tid] = 0u;
            unsigned int x = c;   // inclusive scan over the wave
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const unsigned int y = __shfl_up(x, off, 64);
                if (lane >= off) x += y;
            }
            if (lane == 63) wsum[wave] = x;
            __syncthreads();
            unsigned int incl = x;
            for (int w = 0; w < wave; ++w) incl += wsum[w];
            const unsigned int excl = incl - c;
            if (rank >= excl && rank < incl) { s_bin = (unsigned int)tid; s_rank = rank - excl; }   // (exactly one thread: rank < n)
            __syncthreads();
            prefix |= (unsigned long long)s_bin << shift_bits;
            rank = s_rank;
        }
        unsigned long long upper = prefix;
        if (g != 0.0) {
            // s[lo + 1]: the same key when more than lo + 1 keys are <= it, else the smallest key above it (lo + 1 <= m - 1 when g != 0)
            unsigned int le = 0u;
            unsigned long long above = STAT_KEY_OUT;
            for (int32_t i = tid; i < n; i += STAT_THREADS) {
                const unsigned long long key = key_at(i);
                if (key <= prefix) ++le;
                else if (key < above) above = key;
            }
            atomicAdd(&s_le, le);
            atomicMin(&s_above, above);
            __syncthreads();
            if (s_le <= (unsigned int)lo + 1u) upper = s_above;
        }
        if (tid == 0) out[NYX_HIP_STAT_FIXED + j] = stat_quantile_value(stat_unkey(prefix), stat_unkey(upper), g);
        __syncthreads();   // (s_le / s_above are reset by the next probability)
    }
}

}  // namespace

// (row, sample) pairs beyond the grid are walked by the same workgroup, one after the other
extern "C" __global__ __launch_bounds__(STAT_THREADS) void nyxstat_lds_kernel(StatArgs a, int64_t total) {
    for (int64_t rk = blockIdx.x; rk < total; rk += gridDim.x) {
        stat_block<true>(a, rk);
        __syncthreads();
    }
}

extern "C" __global__ __launch_bounds__(STAT_THREADS) void nyxstat_global_kernel(StatArgs a, int64_t total) {
    for (int64_t rk = blockIdx.x; rk < total; rk += gridDim.x) {
        stat_block<false>(a, rk);
        __syncthreads();
    }
}

extern "C" hipError_t nyx_launch_series_stats(const StatArgs *args, int64_t n_rows, hipStream_t stream) {
    StatArgs a = *args;
    const int64_t total = n_rows * a.capacity;
    const unsigned grid = (unsigned)(total < (int64_t)(1 << 20) ? total : (int64_t)(1 << 20));
    if (a.n <= STAT_LDS_KEYS) {
        const size_t bytes = (size_t)a.n * sizeof(unsigned long long);
        if (bytes > 48 * 1024) {
            const hipError_t e = hipFuncSetAttribute((const void *)nyxstat_lds_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                     STAT_LDS_KEYS * (int)sizeof(unsigned long long));
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(nyxstat_lds_kernel, dim3(grid), dim3(STAT_THREADS), bytes, stream, a, total);
    } else {
        hipLaunchKernelGGL(nyxstat_global_kernel, dim3(grid), dim3(STAT_THREADS), 0, stream, a, total);
    }
    return hipGetLastError();
}
