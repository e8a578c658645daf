// stats_args.h — launch arguments of the statistics kernel (stats_kernel.hip), shared with abi.cpp (host and device; no HIP).
#pragma once
#include <stdint.h>

#include "../../include/nyx_hip_stats.h"

// one workgroup per (row, sample): four waves
#define STAT_THREADS 256
// The most keys of one (row, sample) the kernel parks in dynamic LDS: 128 KiB of the CU's 160 KiB, beside 1.2 KiB of static LDS.
// A block with more runs takes its keys from the row in global memory, pass after pass (the same selection, another key source).
#define STAT_LDS_KEYS 16384

struct StatArgs {
    const double *values;   // [n_rows][capacity][n]
    const int32_t *len;     // [n]
    const int32_t *status;  // [n], or NULL
    double *stats;          // [n_rows][capacity][NYX_HIP_STAT_FIXED + q.n_probs]
    int64_t capacity;
    int32_t n;
    int32_t _pad;
    nyx_hip_stats_query_t q;
};
