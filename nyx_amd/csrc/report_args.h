// report_args.h — launch arguments of the report kernels (report_kernel.hip), shared with abi.cpp.
#pragma once
#include <stdint.h>

#include "../../include/nyx_hip_reports.h"

// shared intermediates of one sample: each is computed once, and only when a requested parameter needs it
enum { REP_NEED_R = 1, REP_NEED_V = 2, REP_NEED_H = 4, REP_NEED_ENERGY = 8, REP_NEED_SMA = 16, REP_NEED_EVEC = 32 };

struct ValuesArgs {
    nyx_hip_traj_t src;   // device pointers, step-major [k * n + i]
    int64_t n;            // trajectories
    int64_t capacity;     // stored samples per trajectory and parameter
    double *values;       // [n_params][capacity][n]
    int32_t *len;         // [n] samples produced
    nyx_hip_values_query_t q;  // (mu resolved by the caller: > 0)
    int32_t need;              // REP_NEED_* of q.param[0 .. n_params), filled by the launcher
    int64_t samples_per_block; // filled by the launcher
};

// REP_NEED_* of one parameter; -1 = not a parameter of enum nyx_hip_state_param
static inline int32_t report_param_needs(int32_t param) {
    switch (param) {
    case NYX_HIP_SP_X: case NYX_HIP_SP_Y: case NYX_HIP_SP_Z: case NYX_HIP_SP_VX: case NYX_HIP_SP_VY: case NYX_HIP_SP_VZ: return 0;
    case NYX_HIP_SP_RMAG: return REP_NEED_R;
    case NYX_HIP_SP_VMAG: return REP_NEED_V;
    case NYX_HIP_SP_HMAG: case NYX_HIP_SP_INCLINATION: case NYX_HIP_SP_RAAN: return REP_NEED_H;
    case NYX_HIP_SP_ENERGY: return REP_NEED_R | REP_NEED_V | REP_NEED_ENERGY;
    case NYX_HIP_SP_SEMI_MAJOR_AXIS: case NYX_HIP_SP_PERIOD: return REP_NEED_R | REP_NEED_V | REP_NEED_ENERGY | REP_NEED_SMA;
    case NYX_HIP_SP_ECCENTRICITY: return REP_NEED_R | REP_NEED_V | REP_NEED_EVEC;
    case NYX_HIP_SP_APOAPSIS_RADIUS: case NYX_HIP_SP_PERIAPSIS_RADIUS:
        return REP_NEED_R | REP_NEED_V | REP_NEED_ENERGY | REP_NEED_SMA | REP_NEED_EVEC;
    case NYX_HIP_SP_AOP: case NYX_HIP_SP_TRUE_ANOMALY: return REP_NEED_R | REP_NEED_V | REP_NEED_H | REP_NEED_EVEC;
    default: return -1;
    }
}
