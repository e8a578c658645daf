// ric_args.h — launch arguments of the RIC kernels (ric_kernel.hip), shared with abi.cpp.
#pragma once
#include <stdint.h>

#include "../../include/nyx_hip_ric.h"

struct RicArgs {
    nyx_hip_traj_t src;   // the runs: device pointers, step-major [k * n + i]
    nyx_hip_traj_t ref;   // the reference trajectories: step-major [k * n_ref + j], j = 0 (n_ref = 1) or i (n_ref = n)
    int64_t n, n_ref;
    int64_t capacity;     // stored samples per run and component
    double *values;       // [6][capacity][n]
    int32_t *len;         // [n] samples produced
    int64_t *epoch0;      // [n] epoch of sample 0, or NULL
    double *moments;      // [capacity][NYX_HIP_RIC_MOMENTS], or NULL
    nyx_hip_ric_query_t q;
    int64_t samples_per_block;  // filled by the launcher
};
