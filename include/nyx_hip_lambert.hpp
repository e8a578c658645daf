// nyx_hip_lambert.hpp — thin C++17 wrapper of include/nyx_hip_lambert.h, beside nyx_hip_frame.hpp: a batch of Lambert problems and a
// departure x arrival grid (a porkchop) whose body states come from the context's ephemerides, up to eight parameters per launch.
#pragma once
#include <limits>
#include <stdexcept>
#include <vector>

#include "nyx_hip.hpp"
#include "nyx_hip_lambert.h"

namespace nyx {

// The solver's settings: the reference's defaults
struct LambertSolver {
    int32_t way = NYX_HIP_LMB_AUTO;
    int32_t n_revs = 0;
    int32_t high_path = 0;
    int32_t max_iter = NYX_HIP_LMB_MAX_ITER;
    double tol = 1e-4;
};

// values[(p * n_dep + i) * n_arr + j]: parameter p of departure i and arrival j; status[i * n_arr + j] (a batch is one row: n_dep = 1)
struct LambertGrid {
    int64_t n_dep = 0, n_arr = 0;
    std::vector<int32_t> params;   // enum nyx_hip_lambert_param
    std::vector<double> values;
    std::vector<int32_t> status;   // enum nyx_hip_lambert_status
    double at(size_t p, int64_t i, int64_t j) const { return values[(p * (size_t)n_dep + (size_t)i) * (size_t)n_arr + (size_t)j]; }
};

namespace detail {
inline nyx_hip_lambert_query_t lambert_query(const std::vector<int32_t> &params, const LambertSolver &s) {
    if (params.size() < 1 || params.size() > NYX_HIP_MAX_LAMBERT_PARAMS) throw std::invalid_argument("lambert: 1 .. 8 parameters per call");
    nyx_hip_lambert_query_t q{};
    q.n_params = (int32_t)params.size();
    for (size_t k = 0; k < params.size(); ++k) q.param[k] = params[k];
    q.way = s.way;
    q.n_revs = s.n_revs;
    q.high_path = s.high_path;
    q.max_iter = s.max_iter;
    q.tol = s.tol;
    return q;
}
}  // namespace detail

// n problems: rv1 / rv2 component-major [6][n] (the bodies' full states), tof_s [n]
inline LambertGrid lambert_batch(GpuPropagator &prop, const std::vector<double> &rv1, const std::vector<double> &rv2, const std::vector<double> &tof_s,
                                 double mu_km3_s2, const std::vector<int32_t> &params, const LambertSolver &solver = {}) {
    const size_t n = tof_s.size();
    if (rv1.size() != 6 * n || rv2.size() != 6 * n) throw std::invalid_argument("lambert_batch: rv1 and rv2 hold 6 n doubles");
    const nyx_hip_lambert_query_t q = detail::lambert_query(params, solver);
    LambertGrid out;
    out.n_dep = 1;
    out.n_arr = (int64_t)n;
    out.params = params;
    out.values.assign(params.size() * n, std::numeric_limits<double>::quiet_NaN());
    out.status.assign(n, 0);
    if (nyx_hip_lambert_batch(prop.raw(), rv1.data(), rv2.data(), tof_s.data(), (int64_t)n, mu_km3_s2, &q, out.values.data(), out.status.data()) != NYX_HIP_RC_OK)
        throw std::runtime_error(nyx_hip_last_error());
    return out;
}

// The porkchop of `q` (its chains, epochs and mu filled by the caller; `q.solve` is overwritten from `params` and `solver`)
inline LambertGrid lambert_grid(GpuPropagator &prop, nyx_hip_lambert_grid_query_t q, const std::vector<int32_t> &params, const LambertSolver &solver = {}) {
    q.solve = detail::lambert_query(params, solver);
    if (q.n_dep < 0 || q.n_arr < 0) throw std::invalid_argument("lambert_grid: negative size");
    LambertGrid out;
    out.n_dep = q.n_dep;
    out.n_arr = q.n_arr;
    out.params = params;
    const size_t cells = (size_t)q.n_dep * (size_t)q.n_arr;
    out.values.assign(params.size() * cells, std::numeric_limits<double>::quiet_NaN());
    out.status.assign(cells, 0);
    if (nyx_hip_lambert_grid(prop.raw(), &q, out.values.data(), out.status.data()) != NYX_HIP_RC_OK) throw std::runtime_error(nyx_hip_last_error());
    return out;
}

}  // namespace nyx
