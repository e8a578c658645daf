// The refusal cases of the sampled-series entries (series_host_check.cpp): one line per case - the case's name, the return code, the
// message or "-".  `V` supplies the validators under test as static members returning an Outcome:
//   traj(t, what, need_epochs), eval(ctx, traj, n, query, m, step_ns, out, status, mode),
//   values(ctx, traj, n, q, capacity, values, len), gt(the same with a nyx_hip_gt_query_t),
//   ric(ctx, traj, n, ref, n_ref, q, capacity, values, len)
// so that the same table can be run through another implementation of them (tests/golden/series_check.txt was written that way).
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>

#include "../../include/nyx_hip_groundtrack.h"
#include "../../include/nyx_hip_reports.h"
#include "../../include/nyx_hip_ric.h"

struct nyx_hip_ctx { int unused; };  // (the validators only ask whether there is one)
struct Outcome { int rc; std::string msg; };

// what the non-null arguments point at (nothing reads through them)
static int64_t i64[4];
static double f64[4];
static int32_t i32[4];
static nyx_hip_ctx the_ctx;

template <typename V> void series_refusal_cases(std::FILE *f) {
    nyx_hip_ctx *const ctx = &the_ctx;
    const nyx_hip_traj_t good = {4, i64, f64, f64, f64, f64, f64, f64, i32};
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const int64_t cap_max = 2147483647LL;
    auto put = [&](const std::string &name, const Outcome &o) { std::fprintf(f, "%s %d %s\n", name.c_str(), o.rc, o.msg.empty() ? "-" : o.msg.c_str()); };
    auto num = [](const char *stem, long long k) { return std::string(stem) + std::to_string(k); };

    // ---- check_traj
    {
        put("traj.good", V::traj(&good, "traj", true));
        put("traj.null", V::traj(nullptr, "traj", true));
        nyx_hip_traj_t t = good;
        t.capacity = -1; put("traj.capacity-1", V::traj(&t, "out", true));
        t = good; t.capacity = 0; put("traj.capacity0", V::traj(&t, "traj", true));
        t = good; t.epoch_ns = nullptr; put("traj.no_epochs.needed", V::traj(&t, "ref", true));
        put("traj.no_epochs.not_needed", V::traj(&t, "ref", false));
        t = good; t.x_km = nullptr; put("traj.no_x", V::traj(&t, "traj", true));
        t = good; t.y_km = nullptr; put("traj.no_y", V::traj(&t, "traj", true));
        t = good; t.z_km = nullptr; put("traj.no_z", V::traj(&t, "traj", true));
        t = good; t.vx_km_s = nullptr; put("traj.no_vx", V::traj(&t, "traj", true));
        t = good; t.vy_km_s = nullptr; put("traj.no_vy", V::traj(&t, "traj", true));
        t = good; t.vz_km_s = nullptr; put("traj.no_vz", V::traj(&t, "traj", false));
        t = good; t.len = nullptr; put("traj.no_len", V::traj(&t, "traj", false));
    }

    nyx_hip_traj_t bad = good;
    bad.len = nullptr;

    // ---- traj_at (mode 0) / traj_every (mode 1) on device arrays
    {
        const int AT = 0, EVERY = 1;
        put("eval.at.good", V::eval(ctx, &good, 3, i64, 4, 0, &good, i32, AT));
        put("eval.at.m0_no_arrays", V::eval(ctx, &good, 3, nullptr, 0, 0, &good, nullptr, AT));
        put("eval.at.n0", V::eval(ctx, &good, 0, i64, 2, 0, &good, i32, AT));
        put("eval.every.good", V::eval(ctx, &good, 3, nullptr, 0, 1, &good, nullptr, EVERY));
        put("eval.null_ctx", V::eval(nullptr, &good, 3, i64, 2, 0, &good, i32, AT));
        put("eval.null_ctx+bad_traj", V::eval(nullptr, &bad, 3, i64, 2, 0, &good, i32, AT));
        put("eval.bad_traj", V::eval(ctx, &bad, 3, i64, 2, 0, &good, i32, AT));
        put("eval.null_traj", V::eval(ctx, nullptr, 3, nullptr, 0, 60, &good, nullptr, EVERY));
        put("eval.bad_out", V::eval(ctx, &good, 3, i64, 2, 0, &bad, i32, AT));
        put("eval.bad_traj+bad_out", V::eval(ctx, &bad, 3, i64, 2, 0, &bad, i32, AT));
        put("eval.bad_out+negative_n", V::eval(ctx, &good, -1, i64, 2, 0, nullptr, i32, AT));
        put("eval.negative_n", V::eval(ctx, &good, -1, i64, 2, 0, &good, i32, AT));
        put("eval.every.negative_n+step0", V::eval(ctx, &good, -1, nullptr, 0, 0, &good, nullptr, EVERY));
        put("eval.at.negative_n+m-1", V::eval(ctx, &good, -2, i64, -1, 0, &good, i32, AT));
        put("eval.at.m-1", V::eval(ctx, &good, 3, i64, -1, 0, &good, i32, AT));
        put("eval.at.no_query", V::eval(ctx, &good, 3, nullptr, 2, 0, &good, i32, AT));
        put("eval.at.no_status", V::eval(ctx, &good, 3, i64, 2, 0, &good, nullptr, AT));
        put("eval.at.m_eq_capacity", V::eval(ctx, &good, 3, i64, 4, 0, &good, i32, AT));
        put("eval.at.m_gt_capacity", V::eval(ctx, &good, 3, i64, 5, 0, &good, i32, AT));
        put("eval.at.no_query+m_gt_capacity", V::eval(ctx, &good, 3, nullptr, 5, 0, &good, i32, AT));
        put("eval.at.step_ignored", V::eval(ctx, &good, 3, i64, 2, -7, &good, i32, AT));
        put("eval.every.step0", V::eval(ctx, &good, 3, nullptr, 0, 0, &good, nullptr, EVERY));
        put("eval.every.step-1", V::eval(ctx, &good, 3, nullptr, 0, -1, &good, nullptr, EVERY));
        put("eval.every.n0+step0", V::eval(ctx, &good, 0, nullptr, 0, 0, &good, nullptr, EVERY));
        put("eval.every.m_ignored", V::eval(ctx, &good, 3, nullptr, 9, 60, &good, nullptr, EVERY));
    }

    // ---- the StateParameter series
    {
        nyx_hip_values_query_t base;
        std::memset(&base, 0, sizeof base);
        base.n_params = 2; base.param[0] = NYX_HIP_SP_X; base.param[1] = NYX_HIP_SP_RMAG; base.step_ns = 60;
        auto run = [&](const std::string &name, const nyx_hip_values_query_t &q, nyx_hip_ctx *c = &the_ctx, const nyx_hip_traj_t *t = nullptr,
                       int64_t n = 3, int64_t capacity = 5, double *values = f64, int32_t *len = i32) {
            put("values." + name, V::values(c, t ? t : &good, n, &q, capacity, values, len));
        };
        nyx_hip_values_query_t q = base;
        run("good", q);
        run("n0", q, ctx, nullptr, 0);
        run("n0+no_values", q, ctx, nullptr, 0, 5, nullptr);
        run("null_ctx", q, nullptr);
        run("null_ctx+bad_traj", q, nullptr, &bad);
        run("bad_traj", q, ctx, &bad);
        put("values.null_traj", V::values(ctx, nullptr, 3, &q, 5, f64, i32));
        put("values.bad_traj+null_query", V::values(ctx, &bad, 3, nullptr, 5, f64, i32));
        put("values.null_query", V::values(ctx, &good, 3, nullptr, 5, f64, i32));
        put("values.null_query+negative_n", V::values(ctx, &good, -1, nullptr, 5, f64, i32));
        run("negative_n", q, ctx, nullptr, -1);
        q = base; q.n_params = 0; run("negative_n+n_params0", q, ctx, nullptr, -1);
        run("n_params0", q);
        q.n_params = -3; run("n_params-3", q);
        q = base; q.n_params = NYX_HIP_MAX_REPORT_PARAMS; run("n_params_max", q);
        q.n_params = NYX_HIP_MAX_REPORT_PARAMS + 1; run("n_params_max+1", q);
        q.step_ns = 0; run("n_params_max+1+step0", q);
        q = base; q.n_params = 1; run("n_params1", q);
        for (int p = -1; p <= NYX_HIP_SP_COUNT; ++p) { q = base; q.n_params = 1; q.param[0] = p; run(num("param", p), q); }
        q = base; q.n_params = 4; q.param[2] = 99; q.param[3] = -5; run("param[2]_first_of_two", q);
        q.step_ns = -1; run("param[2]+step-1", q);
        q = base; q.param[5] = 99; run("param_past_n_params_unread", q);
        q = base; q.step_ns = 0; run("step0", q);
        q.step_ns = -5; run("step-5", q);
        run("step-5+capacity0", q, ctx, nullptr, 3, 0);
        q = base;
        run("capacity0", q, ctx, nullptr, 3, 0);
        run("capacity-1", q, ctx, nullptr, 3, -1);
        run("capacity1", q, ctx, nullptr, 3, 1);
        run("capacity_max", q, ctx, nullptr, 3, cap_max);
        run("capacity_max+1", q, ctx, nullptr, 3, cap_max + 1);
        run("capacity0+no_values", q, ctx, nullptr, 3, 0, nullptr);
        run("no_values", q, ctx, nullptr, 3, 5, nullptr);
        run("no_len", q, ctx, nullptr, 3, 5, f64, nullptr);
        q.mu_km3_s2 = -1.0; run("mu_not_checked", q);
    }

    // ---- the ground tracks
    {
        nyx_hip_gt_query_t base;
        std::memset(&base, 0, sizeof base);
        base.n_params = 2; base.param[0] = NYX_HIP_GT_LATITUDE; base.param[1] = NYX_HIP_GT_LONGITUDE; base.step_ns = 60;
        base.frame.kind = NYX_HIP_ROT_IAU; base.frame_eq_radius_km = 6378.0; base.frame_flattening = 0.003;
        auto run = [&](const std::string &name, const nyx_hip_gt_query_t &q, nyx_hip_ctx *c = &the_ctx, const nyx_hip_traj_t *t = nullptr,
                       int64_t n = 3, int64_t capacity = 5, double *values = f64, int32_t *len = i32) {
            put("gt." + name, V::gt(c, t ? t : &good, n, &q, capacity, values, len));
        };
        nyx_hip_gt_query_t q = base;
        run("good", q);
        run("n0", q, ctx, nullptr, 0);
        run("n0+no_len", q, ctx, nullptr, 0, 5, f64, nullptr);
        run("null_ctx", q, nullptr);
        run("null_ctx+bad_traj", q, nullptr, &bad);
        run("bad_traj", q, ctx, &bad);
        put("gt.bad_traj+null_query", V::gt(ctx, &bad, 3, nullptr, 5, f64, i32));
        put("gt.null_query", V::gt(ctx, &good, 3, nullptr, 5, f64, i32));
        put("gt.null_query+negative_n", V::gt(ctx, &good, -1, nullptr, 5, f64, i32));
        run("negative_n", q, ctx, nullptr, -1);
        q = base; q.n_params = 0; run("negative_n+n_params0", q, ctx, nullptr, -1);
        run("n_params0", q);
        q = base; q.n_params = NYX_HIP_MAX_GT_PARAMS; run("n_params_max", q);
        q.n_params = NYX_HIP_MAX_GT_PARAMS + 1; run("n_params_max+1", q);
        q.step_ns = 0; run("n_params_max+1+step0", q);
        for (int p = -1; p <= NYX_HIP_GT_COUNT; ++p) { q = base; q.n_params = 1; q.param[0] = p; run(num("param", p), q); }
        q = base; q.n_params = 3; q.param[1] = 77; q.param[2] = -1; run("param[1]_first_of_two", q);
        q.step_ns = 0; run("param[1]+step0", q);
        q = base; q.step_ns = 0; run("step0", q);
        run("step0+capacity0", q, ctx, nullptr, 3, 0);
        q.frame.kind = NYX_HIP_ROT_EULER_CHEBY; run("step0+kind", q);
        q = base;
        run("capacity0", q, ctx, nullptr, 3, 0);
        run("capacity1", q, ctx, nullptr, 3, 1);
        run("capacity_max", q, ctx, nullptr, 3, cap_max);
        run("capacity_max+1", q, ctx, nullptr, 3, cap_max + 1);
        q.frame.kind = NYX_HIP_ROT_EULER_CHEBY; run("capacity0+kind", q, ctx, nullptr, 3, 0);
        run("kind_euler", q);
        q.frame.n_nut_prec = -1; run("kind+n_nut_prec", q);
        q = base; q.frame.kind = 7; run("kind7", q);
        q = base; q.frame.n_nut_prec = -1; run("n_nut_prec-1", q);
        q.frame_eq_radius_km = 0.0; run("n_nut_prec+radius", q);
        q = base; q.frame.n_nut_prec = 0; run("n_nut_prec0", q);
        q.frame.n_nut_prec = NYX_HIP_MAX_NUT_PREC; run("n_nut_prec_max", q);
        q.frame.n_nut_prec = NYX_HIP_MAX_NUT_PREC + 1; run("n_nut_prec_max+1", q);
        q = base; q.frame_eq_radius_km = 0.0; run("radius0.latitude", q);
        q.frame_flattening = 1.0; run("radius0+flattening1", q);
        q = base; q.frame_eq_radius_km = -1.0; q.n_params = 1; q.param[0] = NYX_HIP_GT_HEIGHT; run("radius-1.height", q);
        q.frame_eq_radius_km = nan; run("radius_nan.height", q);
        q.frame_eq_radius_km = 0.0; q.param[0] = NYX_HIP_GT_LONGITUDE; run("radius0.longitude_only", q);
        q.param[0] = NYX_HIP_GT_RMAG; run("radius0.rmag_only", q);
        q.n_params = 2; q.param[1] = NYX_HIP_GT_HEIGHT; run("radius0.rmag+height", q);
        q = base; q.frame_flattening = 0.0; run("flattening0", q);
        q.frame_flattening = 0.999; run("flattening0.999", q);
        q.frame_flattening = 1.0; run("flattening1", q);
        q.frame_flattening = -0.1; run("flattening-0.1", q);
        q.frame_flattening = nan; run("flattening_nan", q);
        run("flattening+no_values", q, ctx, nullptr, 3, 5, nullptr);
        q = base;
        run("no_values", q, ctx, nullptr, 3, 5, nullptr);
        run("no_len", q, ctx, nullptr, 3, 5, f64, nullptr);
        q.has_frame = 0; q.frame.kind = NYX_HIP_ROT_EULER_CHEBY; run("kind_checked_without_has_frame", q);
    }

    // ---- the RIC dispersions
    {
        nyx_hip_ric_query_t base;
        std::memset(&base, 0, sizeof base);
        base.step_ns = 60; base.frame_of = 1; base.transport = 1; base.smooth_window = 5;
        auto run = [&](const std::string &name, const nyx_hip_ric_query_t &q, int64_t n = 3, int64_t n_ref = 1, int64_t capacity = 5,
                       double *values = f64, int32_t *len = i32, const nyx_hip_traj_t *t = nullptr, const nyx_hip_traj_t *ref = nullptr,
                       nyx_hip_ctx *c = &the_ctx) {
            put("ric." + name, V::ric(c, t ? t : &good, n, ref ? ref : &good, n_ref, &q, capacity, values, len));
        };
        nyx_hip_ric_query_t q = base;
        run("good", q);
        run("null_ctx", q, 3, 1, 5, f64, i32, nullptr, nullptr, nullptr);
        run("null_ctx+bad_traj", q, 3, 1, 5, f64, i32, &bad, nullptr, nullptr);
        run("bad_traj", q, 3, 1, 5, f64, i32, &bad);
        run("bad_ref", q, 3, 1, 5, f64, i32, nullptr, &bad);
        run("bad_traj+bad_ref", q, 3, 1, 5, f64, i32, &bad, &bad);
        put("ric.null_ref", V::ric(ctx, &good, 3, nullptr, 1, &q, 5, f64, i32));
        put("ric.bad_ref+null_query", V::ric(ctx, &good, 3, &bad, 1, nullptr, 5, f64, i32));
        put("ric.null_query", V::ric(ctx, &good, 3, &good, 1, nullptr, 5, f64, i32));
        put("ric.null_query+negative_n", V::ric(ctx, &good, -1, &good, 1, nullptr, 5, f64, i32));
        run("negative_n", q, -1);
        run("negative_n+n_ref", q, -1, 4);
        run("n_ref_one", q, 3, 1);
        run("n_ref_per_run", q, 3, 3);
        run("n_ref0", q, 3, 0);
        run("n_ref2", q, 3, 2);
        run("n_ref4", q, 3, 4);
        run("n0.n_ref0", q, 0, 0);
        run("n0.n_ref1", q, 0, 1);
        run("n0.n_ref2", q, 0, 2);
        run("n0.no_len", q, 0, 1, 3, f64, nullptr);
        q.step_ns = 0; run("n_ref+step0", q, 3, 2);
        run("step0", q);
        run("step0+capacity0", q, 3, 1, 0);
        q.step_ns = -60; run("step-60", q);
        q = base;
        run("capacity0", q, 3, 1, 0);
        run("capacity-1", q, 3, 1, -1);
        run("capacity1", q, 3, 1, 1);
        run("capacity_max", q, 3, 1, cap_max);
        run("capacity_max+1", q, 3, 1, cap_max + 1);
        q.frame_of = 2; run("capacity0+frame_of", q, 3, 1, 0);
        run("frame_of2", q);
        q.transport = 2; run("frame_of+transport", q);
        q = base; q.frame_of = -1; run("frame_of-1", q);
        q.frame_of = 0; run("frame_of0", q);
        q.frame_of = 1; run("frame_of1", q);
        q = base; q.transport = -1; run("transport-1", q);
        q.transport = 2; run("transport2", q);
        q.smooth_window = 4; run("transport+smooth_window", q);
        q.transport = 0; q.smooth_window = 5; run("transport0", q);
        for (int w : {-1, 0, 1, 2, 3, 4, 5, 7, 9, 10, 11}) { q = base; q.smooth_window = w; run(num("smooth_window", w), q); }
        q = base; q.smooth_window = 4; run("smooth_window+no_values", q, 3, 1, 5, nullptr);
        q = base;
        run("no_values", q, 3, 1, 5, nullptr);
        run("no_len", q, 3, 1, 5, f64, nullptr);
        run("no_values_no_len", q, 3, 1, 5, nullptr, nullptr);
    }
}
