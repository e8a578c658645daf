// stats_dev.h — what the statistics kernel (stats_kernel.hip) decides per value, written so that the SAME TEXT compiles for the device
// and for the host (STAT_FN): tests/cxx/stats_host_check.cpp runs it on the CPU.  No HIP includes, nothing read from the process.
//   stat_key / stat_unkey     the monotone 64-bit key of a double and back: unsigned order of the keys = the total order of
//                             include/nyx_hip_stats.h (-inf < finite < +inf, -0.0 before +0.0)
//   stat_key_of               the key of one slot: STAT_KEY_OUT for a run that is not held or whose value is NaN - above every key of C,
//                             so that rank j < |C| of ALL n keys is rank j of C and the selection needs no compaction
//   stat_quantile_rank/_value the quantile formula: h = (m - 1) p, lo = floor(h), g = h - lo; s[lo] when g == 0 or s[lo] == s[lo + 1],
//                             else s[lo] + g (s[lo + 1] - s[lo]); a NaN result is the one quiet NaN
//   stat_ordered_sums         (host) the summation order of the kernel: lane t of STAT_THREADS adds its slots t, t + STAT_THREADS, ..
//                             in that order, a butterfly (xor 32, 16, .. 1) adds the 64 lanes of a wave, the waves are added in index order
// Only + - x and comparisons: compile with -ffp-contract=off and device and host agree to the last bit.
#pragma once
#include <math.h>
#include <stdint.h>

#include "stats_args.h"

#if defined(__HIPCC__)
#define STAT_FN __host__ __device__ static inline
#else
#define STAT_FN static inline
#endif

#define STAT_KEY_OUT 0xFFFFFFFFFFFFFFFFull   // (the key of a NaN: never a key of C)
#define STAT_NAN_BITS 0x7FF8000000000000ull

STAT_FN uint64_t stat_bits(double v) {
    union { double d; uint64_t u; } x;
    x.d = v;
    return x.u;
}
STAT_FN double stat_double(uint64_t u) {
    union { double d; uint64_t u; } x;
    x.u = u;
    return x.d;
}
STAT_FN uint64_t stat_key(double v) {
    const uint64_t b = stat_bits(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
STAT_FN double stat_unkey(uint64_t key) { return stat_double((key >> 63) ? (key & 0x7FFFFFFFFFFFFFFFull) : ~key); }
// (of a key of C) the value is finite: its exponent is not all ones
STAT_FN bool stat_key_finite(uint64_t key) {
    const uint64_t b = (key >> 63) ? key : ~key;
    return (b & 0x7FF0000000000000ull) != 0x7FF0000000000000ull;
}
// run i holds sample k
STAT_FN bool stat_held(const int32_t *len, const int32_t *status, int64_t capacity, int64_t k, int32_t i) {
    if (status && status[i] != 0) return false;
    const int64_t m = len[i] < capacity ? (int64_t)len[i] : capacity;
    return k < m;
}
STAT_FN uint64_t stat_key_of(double v, bool held) { return (held && v == v) ? stat_key(v) : STAT_KEY_OUT; }

// the two neighbouring ranks of the quantile p of m >= 1 values: *lo, and *lo + 1 when the returned g is not zero
STAT_FN double stat_quantile_rank(int32_t m, double p, int32_t *lo) {
    const double h = (double)(m - 1) * p;
    const double f = floor(h);
    *lo = (int32_t)f;
    return h - f;
}
// a = s[lo], b = s[lo + 1] (read only when g != 0)
STAT_FN double stat_quantile_value(double a, double b, double g) {
    if (g == 0.0 || a == b) return a;
    const double q = a + g * (b - a);
    return q == q ? q : stat_double(STAT_NAN_BITS);
}

#if !defined(__HIP_DEVICE_COMPILE__)
// (host) sum and sumsq of d = v - shift over the slots of F, in the kernel's order; key[i] = stat_key_of of slot i
static inline void stat_ordered_sums(const uint64_t *key, int32_t n, double shift, double *sum, double *sumsq) {
    double acc[STAT_THREADS][2];
    for (int t = 0; t < STAT_THREADS; ++t) acc[t][0] = acc[t][1] = 0.0;
    for (int32_t i = 0; i < n; ++i) {
        if (key[i] == STAT_KEY_OUT || !stat_key_finite(key[i])) continue;
        const double d = stat_unkey(key[i]) - shift;
        acc[i % STAT_THREADS][0] += d;
        acc[i % STAT_THREADS][1] += d * d;
    }
    double total[2] = {0.0, 0.0};
    for (int w = 0; w < STAT_THREADS / 64; ++w)
        for (int c = 0; c < 2; ++c) {
            double v[64], u[64];
            for (int l = 0; l < 64; ++l) v[l] = acc[w * 64 + l][c];
            for (int off = 32; off >= 1; off >>= 1) {
                for (int l = 0; l < 64; ++l) u[l] = v[l] + v[l ^ off];
                for (int l = 0; l < 64; ++l) v[l] = u[l];
            }
            total[c] = w == 0 ? v[0] : total[c] + v[0];
        }
    *sum = total[0];
    *sumsq = total[1];
}
#endif
