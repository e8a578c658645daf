// groundtrack_args.h — launch arguments of the ground-track kernels (groundtrack_kernel.hip), shared with abi.cpp.
#pragma once
#include <stdint.h>

#include "../../include/nyx_hip_groundtrack.h"

// shared intermediates of one sample: each is computed once, and only when a requested parameter needs it
enum { GT_NEED_R = 1, GT_NEED_GEODETIC = 2 };

struct GroundTrackArgs {
    nyx_hip_traj_t src;   // device pointers, step-major [k * n + i]
    int64_t n;            // trajectories
    int64_t capacity;     // stored samples per trajectory and parameter
    double *values;       // [n_params][capacity][n]
    int32_t *len;         // [n] samples produced
    nyx_hip_gt_query_t q;
    int32_t need;              // GT_NEED_* of q.param[0 .. n_params), filled by the launcher
    int64_t samples_per_block; // filled by the launcher
};

// GT_NEED_* of one parameter; -1 = not a parameter of enum nyx_hip_gt_param
static inline int32_t gt_param_needs(int32_t param) {
    switch (param) {
    case NYX_HIP_GT_LATITUDE: case NYX_HIP_GT_HEIGHT: return GT_NEED_GEODETIC;
    case NYX_HIP_GT_RMAG: case NYX_HIP_GT_DECLINATION: return GT_NEED_R;
    case NYX_HIP_GT_LONGITUDE: case NYX_HIP_GT_X: case NYX_HIP_GT_Y: case NYX_HIP_GT_Z: case NYX_HIP_GT_VX: case NYX_HIP_GT_VY:
    case NYX_HIP_GT_VZ: case NYX_HIP_GT_VMAG: return 0;
    default: return -1;
    }
}
