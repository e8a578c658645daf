// nyx_hip_target.hpp — thin C++17 wrapper of include/nyx_hip_target.h, beside nyx_hip_lambert.hpp: the differential-correction
// targeter of a whole batch, the Newton loop kept on the device.
#pragma once
#include <cmath>
#include <limits>
#include <stdexcept>
#include <vector>

#include "nyx_hip.hpp"
#include "nyx_hip_target.h"

namespace nyx {

// The reference's `Variable` (its defaults) and `Objective`
struct TargetVariable {
    int32_t component = NYX_HIP_VARY_VELOCITY_X;
    double perturbation = 1e-4, init_guess = 0.0, max_step = 0.2, max_value = 5.0, min_value = -5.0;
};
struct TargetObjective {
    int32_t param = 0;   // enum nyx_hip_frame_param
    double desired = 0.0, tolerance = 0.0, multiplicative_factor = 1.0, additive_factor = 0.0;
};

struct TargeterSolutions {
    int64_t n = 0;
    int32_t iterations_run = 0;
    std::vector<int32_t> status, iterations;       // enum nyx_hip_target_status; the iteration each run ended at
    std::vector<double> correction, achieved_errors;   // [V][n], [O][n]
    StateBatch corrected{0}, achieved{0};
    double correction_at(size_t j, int64_t i) const { return correction[j * (size_t)n + (size_t)i]; }
    double converged_fraction() const {
        size_t ok = 0;
        for (int32_t s : status) ok += s == NYX_HIP_TGT_OK_CONVERGED;
        return n ? (double)ok / (double)n : 0.0;
    }
};

// `q`: the epochs, the frame, the objective target's chain and mu filled by the caller; variables and objectives are written from the lists
inline TargeterSolutions target_batch(GpuPropagator &prop, StateBatch &in, nyx_hip_target_query_t q, const std::vector<TargetVariable> &vars,
                                      const std::vector<TargetObjective> &objs) {
    if (vars.size() < 1 || vars.size() > NYX_HIP_MAX_TARGET_VARS || objs.size() < 1 || objs.size() > NYX_HIP_MAX_TARGET_OBJS)
        throw std::invalid_argument("target_batch: 1 .. 6 variables and 1 .. 6 objectives");
    q.n_vars = (int32_t)vars.size();
    q.n_objs = (int32_t)objs.size();
    for (size_t j = 0; j < vars.size(); ++j) {
        q.var_component[j] = vars[j].component; q.var_perturbation[j] = vars[j].perturbation; q.var_init_guess[j] = vars[j].init_guess;
        q.var_max_step[j] = vars[j].max_step; q.var_max_value[j] = vars[j].max_value; q.var_min_value[j] = vars[j].min_value;
    }
    for (size_t o = 0; o < objs.size(); ++o) {
        q.obj_param[o] = objs[o].param; q.obj_desired[o] = objs[o].desired; q.obj_tolerance[o] = objs[o].tolerance;
        q.obj_mult[o] = objs[o].multiplicative_factor; q.obj_add[o] = objs[o].additive_factor;
    }
    const size_t n = (size_t)in.size();
    TargeterSolutions out;
    out.n = in.size();
    out.status.assign(n, 0);
    out.iterations.assign(n, 0);
    out.correction.assign(vars.size() * n, std::numeric_limits<double>::quiet_NaN());
    out.achieved_errors.assign(objs.size() * n, std::numeric_limits<double>::quiet_NaN());
    out.corrected = StateBatch(in.size());
    out.achieved = StateBatch(in.size());
    nyx_hip_target_result_t res{};
    res.status = out.status.data(); res.iterations = out.iterations.data();
    res.correction = out.correction.data(); res.achieved_errors = out.achieved_errors.data();
    res.corrected = out.corrected.view(); res.achieved = out.achieved.view();
    res.corrected.step_ns = res.achieved.step_ns = nullptr;
    nyx_hip_states_t vin = in.view();
    if (nyx_hip_target_batch(prop.raw(), &vin, &q, &res) != NYX_HIP_RC_OK) throw std::runtime_error(nyx_hip_last_error());
    out.iterations_run = res.iterations_run;
    return out;
}

}  // namespace nyx
