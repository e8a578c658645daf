// The refusal cases of the entries that run the propagator and of the two older host flavours (run_host_check.cpp): one line per
// case - the case's name, the return code, the message or "-".  `V` supplies the argument checks of a whole entry, up to its first
// use of the device, as static members returning an Outcome (rc 0: accepted, or an empty batch, which is done):
//   states(s, what)                                        check_states
//   run(ctx, in, out, stm)                                 propagate_batch / until_epoch; stm: the context carries STMs
//   with_traj(ctx, in, out, traj, stm)                     propagate_batch_with_traj
//   sharded(ctxs, n_ctx, in, out, traj)                    propagate_batch_sharded, before it starts its shards
//   event(ctx, in, event, out, traj, stm)                  propagate_until_event
//   predict(ctx, flags, in, cfg, est, out, hist)           predict_until; flags: the context's
//   moments_device(ctx, s, out55), moments_host(...)       ensemble_moments, both flavours
//   eval_host(ctx, traj, n, query, m, step_ns, out, status, mode)   traj_at (mode 0) / traj_every (mode 1) on host arrays
// so that the same table can be run through another implementation of them (tests/golden/run_check.txt was written that way).
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>

#include "../../include/nyx_hip.h"

struct nyx_hip_ctx { int unused; };  // (the validators only ask whether there is one)
struct Outcome { int rc; std::string msg; };

// what the non-null arguments point at (nothing reads through them)
static int64_t i64[4];
static double f64[4];
static int32_t i32[4];
static nyx_hip_ctx the_ctx;

template <typename V> void run_refusal_cases(std::FILE *f) {
    nyx_hip_ctx *const ctx = &the_ctx;
    const uint32_t STM = NYX_HIP_FLAG_STM;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    auto put = [&](const std::string &name, const Outcome &o) { std::fprintf(f, "%s %d %s\n", name.c_str(), o.rc, o.msg.empty() ? "-" : o.msg.c_str()); };
    // (the return code alone: the one message that may differ between implementations, the host flavour's "negative n")
    auto put_rc = [&](const std::string &name, const Outcome &o) { std::fprintf(f, "%s %d *\n", name.c_str(), o.rc); };
    auto num = [](const char *stem, long long k) { return std::string(stem) + std::to_string(k); };

    nyx_hip_states_t good;  // three trajectories, no STMs
    std::memset(&good, 0, sizeof good);
    good.n = 3; good.epoch_ns = i64;
    good.x_km = good.y_km = good.z_km = good.vx_km_s = good.vy_km_s = good.vz_km_s = f64;
    nyx_hip_states_t with_stm = good, empty = good, bad = good, two = good, four = good;
    with_stm.stm = f64;
    empty.n = 0;
    bad.vy_km_s = nullptr;
    two.n = 2;
    four.n = 4;
    const nyx_hip_traj_t tgood = {4, i64, f64, f64, f64, f64, f64, f64, i32};
    nyx_hip_traj_t tbad = tgood;
    tbad.len = nullptr;
    auto tcap = [&](int64_t capacity) { nyx_hip_traj_t t = tgood; t.capacity = capacity; return t; };

    // ---- check_states
    {
        put("states.good", V::states(&good, "in"));
        put("states.null", V::states(nullptr, "in"));
        put("states.n0", V::states(&empty, "out"));
        nyx_hip_states_t s = good;
        s.n = -1; put("states.n-1", V::states(&s, "out"));
        s = good; s.epoch_ns = nullptr; put("states.no_epochs", V::states(&s, "in"));
        s = empty; s.epoch_ns = nullptr; put("states.n0.no_epochs", V::states(&s, "in"));
        double *nyx_hip_states_t::*const cart[6] = {&nyx_hip_states_t::x_km, &nyx_hip_states_t::y_km, &nyx_hip_states_t::z_km,
                                                    &nyx_hip_states_t::vx_km_s, &nyx_hip_states_t::vy_km_s, &nyx_hip_states_t::vz_km_s};
        for (int k = 0; k < 6; ++k) { s = good; s.*cart[k] = nullptr; put(num("states.no_cart", k), V::states(&s, "out")); }
        s = good; s.cr = s.cd = s.prop_mass_kg = nullptr; s.stm = nullptr; s.step_ns = nullptr; put("states.optional_rows_null", V::states(&s, "in"));
    }

    // ---- the host bracket: propagate_batch / propagate_until_epoch
    {
        put("run.good", V::run(ctx, &good, &good, false));
        put("run.null_ctx", V::run(nullptr, &good, &good, false));
        put("run.null_ctx+bad_in", V::run(nullptr, &bad, &good, true));
        put("run.null_in", V::run(ctx, nullptr, &good, false));
        put("run.bad_in", V::run(ctx, &bad, &good, false));
        put("run.bad_in+bad_out", V::run(ctx, &bad, &bad, false));
        put("run.null_out", V::run(ctx, &good, nullptr, false));
        put("run.bad_out", V::run(ctx, &good, &bad, false));
        put("run.bad_out+smaller", V::run(ctx, &four, &bad, false));
        put("run.out_smaller", V::run(ctx, &good, &two, false));
        put("run.out_equal", V::run(ctx, &good, &good, false));
        put("run.out_larger", V::run(ctx, &good, &four, false));
        put("run.n0", V::run(ctx, &empty, &good, false));
        put("run.n0.out_n0", V::run(ctx, &empty, &empty, false));
        put("run.n0+bad_out", V::run(ctx, &empty, &bad, false));
        put("run.n0+stm_missing", V::run(ctx, &empty, &empty, true));
        put("run.stm.good", V::run(ctx, &with_stm, &with_stm, true));
        put("run.stm.no_in_stm", V::run(ctx, &good, &with_stm, true));
        put("run.stm.no_out_stm", V::run(ctx, &with_stm, &good, true));
        put("run.stm.out_smaller+no_stm", V::run(ctx, &good, &two, true));
        put("run.stm_given_without_flag", V::run(ctx, &with_stm, &with_stm, false));
    }

    // ---- propagate_batch_with_traj
    {
        const nyx_hip_traj_t t0 = tcap(0), t1 = tcap(1), tneg = tcap(-1);
        put("with_traj.good", V::with_traj(ctx, &good, &good, &tgood, false));
        put("with_traj.null_traj", V::with_traj(ctx, &good, &good, nullptr, false));
        put("with_traj.capacity-1", V::with_traj(ctx, &good, &good, &tneg, false));
        put("with_traj.capacity0", V::with_traj(ctx, &good, &good, &t0, false));
        put("with_traj.capacity1", V::with_traj(ctx, &good, &good, &t1, false));
        put("with_traj.capacity0+null_ctx", V::with_traj(nullptr, &good, &good, &t0, false));
        put("with_traj.null_ctx", V::with_traj(nullptr, &good, &good, &t1, false));
        put("with_traj.capacity0+bad_in", V::with_traj(ctx, &bad, &good, &t0, false));
        put("with_traj.n0+capacity0", V::with_traj(ctx, &empty, &good, &t0, false));
        put("with_traj.n0", V::with_traj(ctx, &empty, &good, &t1, false));
        put("with_traj.null_arrays_pass_here", V::with_traj(ctx, &good, &good, &tbad, false));
        put("with_traj.stm_missing", V::with_traj(ctx, &good, &good, &t1, true));
    }

    // ---- propagate_batch_sharded
    {
        nyx_hip_ctx *one[1] = {ctx}, *three[3] = {ctx, ctx, ctx}, *hole[3] = {ctx, nullptr, ctx}, *holes[3] = {ctx, nullptr, nullptr};
        const nyx_hip_traj_t t0 = tcap(0), t1 = tcap(1);
        put("sharded.good", V::sharded(three, 3, &good, &good, nullptr));
        put("sharded.good.traj", V::sharded(one, 1, &good, &good, &t1));
        put("sharded.null_ctxs", V::sharded(nullptr, 3, &good, &good, nullptr));
        put("sharded.n_ctx0", V::sharded(three, 0, &good, &good, nullptr));
        put("sharded.n_ctx-1", V::sharded(three, -1, &good, &good, nullptr));
        put("sharded.null_in", V::sharded(three, 3, nullptr, &good, nullptr));
        put("sharded.null_out", V::sharded(three, 3, &good, nullptr, nullptr));
        put("sharded.null_out+hole", V::sharded(hole, 3, &good, nullptr, nullptr));
        put("sharded.hole", V::sharded(hole, 3, &good, &good, nullptr));
        put("sharded.hole_past_n_ctx", V::sharded(hole, 1, &good, &good, nullptr));
        put("sharded.first_of_two_holes", V::sharded(holes, 3, &good, &good, nullptr));
        put("sharded.hole+sizes", V::sharded(hole, 3, &good, &four, nullptr));
        put("sharded.out_larger", V::sharded(three, 3, &good, &four, nullptr));
        put("sharded.out_smaller", V::sharded(three, 3, &good, &two, nullptr));
        put("sharded.sizes+capacity0", V::sharded(three, 3, &good, &two, &t0));
        put("sharded.capacity0", V::sharded(three, 3, &good, &good, &t0));
        put("sharded.capacity1", V::sharded(three, 3, &good, &good, &t1));
        put("sharded.n0", V::sharded(three, 3, &empty, &empty, nullptr));
        put("sharded.n0+capacity0", V::sharded(three, 3, &empty, &empty, &t0));
        put("sharded.bad_in_passes_here", V::sharded(three, 3, &bad, &good, nullptr));
    }

    // ---- propagate_until_event
    {
        nyx_hip_event_t base;
        std::memset(&base, 0, sizeof base);
        base.scalar = NYX_HIP_EV_TRUE_ANOMALY_DEG; base.trigger = 1; base.desired = 180.0; base.value_precision = 1e-3; base.epoch_precision_ns = 1000;
        base.frame.kind = NYX_HIP_ROT_IAU; base.frame_eq_radius_km = 6378.0; base.frame_flattening = 0.003;
        auto run = [&](const std::string &name, const nyx_hip_event_t &e, const nyx_hip_traj_t *t = nullptr, const nyx_hip_states_t *in = nullptr,
                       const nyx_hip_states_t *out = nullptr, nyx_hip_ctx *c = &the_ctx, bool stm = false) {
            put("event." + name, V::event(c, in ? in : &good, &e, out ? out : &good, t ? t : &tgood, stm));
        };
        nyx_hip_event_t e = base;
        run("good", e);
        run("null_ctx", e, nullptr, nullptr, nullptr, nullptr);
        put("event.null_event", V::event(ctx, &good, nullptr, &good, &tgood, false));
        put("event.null_event+null_traj", V::event(ctx, &good, nullptr, &good, nullptr, false));
        for (int t : {-1, 0, 1, 2, 3}) { e = base; e.trigger = t; run(num("trigger", t), e); }
        for (int s : {-1, 0, 1, 10, 11, 12, 13, 14, 15}) { e = base; e.scalar = s; run(num("scalar", s), e); }
        e = base; e.value_precision = 0.0; run("value_precision0", e);
        e.value_precision = -1e-9; run("value_precision_negative", e);
        e.value_precision = nan; run("value_precision_nan", e);
        e = base; e.epoch_precision_ns = 0; run("epoch_precision0", e);
        e.epoch_precision_ns = -1; run("epoch_precision-1", e);
        // the observer frame
        e = base; e.has_frame = 1; run("frame.iau", e);
        e.frame.kind = NYX_HIP_ROT_EULER_CHEBY; run("frame.euler", e);
        e.has_frame = 0; run("frame.euler_without_has_frame", e);
        e = base; e.has_frame = 1; e.frame.n_nut_prec = -1; run("frame.n_nut_prec-1", e);
        e.frame.n_nut_prec = 0; run("frame.n_nut_prec0", e);
        e.frame.n_nut_prec = NYX_HIP_MAX_NUT_PREC; run("frame.n_nut_prec_max", e);
        e.frame.n_nut_prec = NYX_HIP_MAX_NUT_PREC + 1; run("frame.n_nut_prec_max+1", e);
        e.trigger = 0; run("frame+trigger", e);
        e = base; e.has_frame = 1; e.frame.kind = NYX_HIP_ROT_EULER_CHEBY; e.scalar = NYX_HIP_EV_HEIGHT_KM; e.frame_eq_radius_km = 0.0; run("frame+ellipsoid", e);
        // the ellipsoid of the geodetic scalars
        for (int s : {NYX_HIP_EV_LATITUDE_DEG, NYX_HIP_EV_HEIGHT_KM}) {
            const std::string g = s == NYX_HIP_EV_LATITUDE_DEG ? "latitude." : "height.";
            e = base; e.scalar = s; run(g + "good", e);
            e.frame_flattening = 0.0; run(g + "flattening0", e);
            e.frame_flattening = 0.9999999999; run(g + "flattening_below1", e);
            e.frame_flattening = 1.0; run(g + "flattening1", e);
            e.frame_flattening = -1e-12; run(g + "flattening_negative", e);
            e.frame_flattening = nan; run(g + "flattening_nan", e);
            e = base; e.scalar = s; e.frame_eq_radius_km = 0.0; run(g + "radius0", e);
            e.frame_eq_radius_km = -1.0; run(g + "radius-1", e);
            e.frame_eq_radius_km = nan; run(g + "radius_nan", e);
            e.trigger = 0; run(g + "radius+trigger", e);
        }
        e = base; e.scalar = NYX_HIP_EV_DECLINATION_DEG; e.frame_eq_radius_km = 0.0; e.frame_flattening = 2.0; run("declination.ellipsoid_unread", e);
        // the trajectory
        const nyx_hip_traj_t t0 = tcap(0), t1 = tcap(1), t2 = tcap(2), tneg = tcap(-1);
        e = base;
        put("event.null_traj", V::event(ctx, &good, &e, &good, nullptr, false));
        run("bad_traj", e, &tbad);
        run("capacity-1", e, &tneg);
        run("capacity0", e, &t0);
        run("capacity1", e, &t1);
        run("capacity2", e, &t2);
        e.trigger = 0; run("trigger+bad_traj", e, &tbad);
        run("trigger+capacity1", e, &t1);
        e = base;
        run("capacity1+bad_in", e, &t1, &bad);
        run("bad_traj+bad_in", e, &tbad, &bad);
        // the batch
        run("bad_in", e, nullptr, &bad);
        put("event.null_in", V::event(ctx, nullptr, &e, &good, &tgood, false));
        run("bad_out", e, nullptr, nullptr, &bad);
        run("out_smaller", e, nullptr, nullptr, &two);
        run("n0", e, nullptr, &empty);
        run("n0+bad_out", e, nullptr, &empty, &bad);
        run("n0+capacity1", e, &t1, &empty);
        e.trigger = 0; run("n0+trigger", e, nullptr, &empty);
        e = base;
        run("stm.good", e, nullptr, &with_stm, &with_stm, ctx, true);
        run("stm.missing", e, nullptr, nullptr, nullptr, ctx, true);
        run("stm.n0+missing", e, nullptr, &empty, nullptr, ctx, true);
        run("stm.out_smaller+missing", e, nullptr, nullptr, &two, ctx, true);
    }

    // ---- predict_until
    {
        nyx_hip_predict_t base;
        std::memset(&base, 0, sizeof base);
        base.max_step_ns = 60; base.end_epoch_ns = 600;
        nyx_hip_estimates_t est = {f64, f64}, est_no_dev = {f64, nullptr}, est_no_covar = {nullptr, f64};
        nyx_hip_predict_history_t hist = {3, i64, f64, f64, f64, f64, i32};
        auto run = [&](const std::string &name, const nyx_hip_predict_t &c, const nyx_hip_predict_history_t *h = nullptr, const nyx_hip_states_t *in = nullptr,
                       const nyx_hip_states_t *out = nullptr, uint32_t flags = NYX_HIP_FLAG_STM, nyx_hip_estimates_t *e = nullptr) {
            put("predict." + name, V::predict(&the_ctx, flags, in ? in : &good, &c, e ? e : &est, out ? out : &good, h));
        };
        nyx_hip_predict_t c = base;
        run("good", c);
        run("good.hist", c, &hist);
        run("good.no_state_dev", c, nullptr, nullptr, nullptr, STM, &est_no_dev);
        run("good.stm_not_needed_in_batch", c, nullptr, &good, &good);
        put("predict.null_ctx", V::predict(nullptr, 0, &good, &c, &est, &good, nullptr));
        put("predict.null_cfg", V::predict(ctx, STM, &good, nullptr, &est, &good, nullptr));
        put("predict.null_est", V::predict(ctx, STM, &good, &c, nullptr, &good, nullptr));
        run("no_covar", c, nullptr, nullptr, nullptr, STM, &est_no_covar);
        run("no_covar+no_flag", c, nullptr, nullptr, nullptr, 0, &est_no_covar);
        run("no_flag", c, nullptr, nullptr, nullptr, 0);
        run("textbook_flag_alone", c, nullptr, nullptr, nullptr, NYX_HIP_FLAG_STM_TEXTBOOK);
        c.max_step_ns = 0; run("no_flag+step0", c, nullptr, nullptr, nullptr, 0);
        run("step0", c);
        c.max_step_ns = -60; run("step-60", c);
        c.n_process_noise = -1; run("step+noise_count", c);
        c = base; c.max_step_ns = 1; run("step1", c);
        for (int k : {-1, 0, 1, NYX_HIP_MAX_PROCESS_NOISE, NYX_HIP_MAX_PROCESS_NOISE + 1}) { c = base; c.n_process_noise = k; run(num("n_process_noise", k), c); }
        for (int fr : {-1, 0, 1, 2, 3}) { c = base; c.n_process_noise = 1; c.process_noise[0].local_frame = fr; run(num("noise_frame", fr), c); }
        c = base; c.n_process_noise = 3; c.process_noise[1].local_frame = 7; c.process_noise[2].local_frame = -2; run("noise_frame.first_of_two", c);
        c = base; c.n_process_noise = 2; c.process_noise[2].local_frame = 9; run("noise_frame.past_count_unread", c);
        c = base; c.n_process_noise = NYX_HIP_MAX_PROCESS_NOISE + 1; c.process_noise[0].local_frame = 9; run("noise_count+noise_frame", c);
        c = base; c.n_process_noise = 1; c.process_noise[0].local_frame = 9;
        nyx_hip_predict_history_t h = hist;
        h.capacity = -1; run("noise_frame+hist", c, &h);
        c = base;
        run("hist.capacity-1", c, &h);
        h.capacity = 0; run("hist.capacity0", c, &h);
        h = hist; h.n_updates = nullptr; run("hist.no_n_updates", c, &h);
        h = hist; h.epoch_ns = nullptr; h.state = h.stm = h.covar = h.state_dev = nullptr; run("hist.only_n_updates", c, &h);
        h.capacity = -1; run("hist.capacity+bad_in", c, &h, &bad);
        run("bad_in", c, nullptr, &bad);
        put("predict.null_in", V::predict(ctx, STM, nullptr, &c, &est, &good, nullptr));
        run("bad_out", c, nullptr, nullptr, &bad);
        put("predict.null_out", V::predict(ctx, STM, &good, &c, &est, nullptr, nullptr));
        run("out_smaller", c, nullptr, nullptr, &two);
        run("n0", c, nullptr, &empty);
        run("n0+bad_out", c, nullptr, &empty, &bad);
        h = hist; h.capacity = -1; run("n0+hist", c, &h, &empty);
        c.max_step_ns = 0; run("n0+step0", c, nullptr, &empty);
    }

    // ---- ensemble_moments, both flavours
    {
        nyx_hip_states_t s = good;
        put("moments.device.good", V::moments_device(ctx, &s, f64));
        put("moments.host.good", V::moments_host(ctx, &s, f64));
        put("moments.device.null_ctx", V::moments_device(nullptr, &s, f64));
        put("moments.host.null_ctx", V::moments_host(nullptr, &s, f64));
        put("moments.device.null_states", V::moments_device(ctx, nullptr, f64));
        put("moments.host.null_states", V::moments_host(ctx, nullptr, f64));
        put("moments.device.null_out", V::moments_device(ctx, &s, nullptr));
        put("moments.host.null_out", V::moments_host(ctx, &s, nullptr));
        put("moments.device.bad_rows", V::moments_device(ctx, &bad, f64));
        put("moments.host.bad_rows", V::moments_host(ctx, &bad, f64));
        put("moments.host.null_out+bad_rows", V::moments_host(ctx, &bad, nullptr));
        s = good; s.epoch_ns = nullptr; s.cr = s.cd = s.prop_mass_kg = nullptr;
        put("moments.device.epochs_and_optional_rows_null", V::moments_device(ctx, &s, f64));
        put("moments.host.epochs_and_optional_rows_null", V::moments_host(ctx, &s, f64));
        s = bad; s.n = 0;
        put("moments.device.n0.bad_rows", V::moments_device(ctx, &s, f64));
        put("moments.host.n0.bad_rows", V::moments_host(ctx, &s, f64));
        s.n = -1;
        put("moments.device.n-1", V::moments_device(ctx, &s, f64));
        put("moments.host.n-1", V::moments_host(ctx, &s, f64));
    }

    // ---- traj_at (mode 0) / traj_every (mode 1) on host arrays
    {
        const int AT = 0, EVERY = 1;
        put("eval_host.at.good", V::eval_host(ctx, &tgood, 3, i64, 4, 0, &tgood, i32, AT));
        put("eval_host.at.m0_no_arrays", V::eval_host(ctx, &tgood, 3, nullptr, 0, 0, &tgood, nullptr, AT));
        put("eval_host.every.good", V::eval_host(ctx, &tgood, 3, nullptr, 0, 60, &tgood, nullptr, EVERY));
        put("eval_host.null_ctx", V::eval_host(nullptr, &tgood, 3, i64, 2, 0, &tgood, i32, AT));
        put("eval_host.null_ctx+bad_traj", V::eval_host(nullptr, &tbad, 0, i64, 2, 0, &tgood, i32, AT));
        put("eval_host.bad_traj", V::eval_host(ctx, &tbad, 3, i64, 2, 0, &tgood, i32, AT));
        put("eval_host.bad_out", V::eval_host(ctx, &tgood, 3, i64, 2, 0, &tbad, i32, AT));
        put("eval_host.bad_traj+bad_out", V::eval_host(ctx, &tbad, 3, i64, 2, 0, &tbad, i32, AT));
        put("eval_host.n0+bad_traj", V::eval_host(ctx, &tbad, 0, i64, 2, 0, &tgood, i32, AT));
        put("eval_host.n0+bad_out", V::eval_host(ctx, &tgood, 0, i64, 2, 0, nullptr, i32, AT));
        put("eval_host.at.n0", V::eval_host(ctx, &tgood, 0, i64, 2, 0, &tgood, i32, AT));
        put("eval_host.at.n0+no_query", V::eval_host(ctx, &tgood, 0, nullptr, 2, 0, &tgood, nullptr, AT));
        put("eval_host.at.n0+m-1", V::eval_host(ctx, &tgood, 0, i64, -1, 0, &tgood, i32, AT));
        put("eval_host.at.n0+m_gt_capacity", V::eval_host(ctx, &tgood, 0, i64, 5, 0, &tgood, i32, AT));
        put("eval_host.every.n0+step0", V::eval_host(ctx, &tgood, 0, nullptr, 0, 0, &tgood, nullptr, EVERY));
        put_rc("eval_host.negative_n", V::eval_host(ctx, &tgood, -1, i64, 2, 0, &tgood, i32, AT));
        put("eval_host.negative_n+bad_out", V::eval_host(ctx, &tgood, -1, i64, 2, 0, &tbad, i32, AT));
        put("eval_host.at.no_query", V::eval_host(ctx, &tgood, 3, nullptr, 2, 0, &tgood, i32, AT));
        put("eval_host.at.no_status", V::eval_host(ctx, &tgood, 3, i64, 2, 0, &tgood, nullptr, AT));
        put("eval_host.at.m-1", V::eval_host(ctx, &tgood, 3, i64, -1, 0, &tgood, i32, AT));
        put("eval_host.at.m_eq_capacity", V::eval_host(ctx, &tgood, 3, i64, 4, 0, &tgood, i32, AT));
        put("eval_host.at.m_gt_capacity", V::eval_host(ctx, &tgood, 3, i64, 5, 0, &tgood, i32, AT));
        put("eval_host.at.no_query+m_gt_capacity", V::eval_host(ctx, &tgood, 3, nullptr, 5, 0, &tgood, i32, AT));
        put("eval_host.every.step0", V::eval_host(ctx, &tgood, 3, nullptr, 0, 0, &tgood, nullptr, EVERY));
        put("eval_host.every.step-1", V::eval_host(ctx, &tgood, 3, nullptr, 0, -1, &tgood, nullptr, EVERY));
        put("eval_host.every.m_ignored", V::eval_host(ctx, &tgood, 3, nullptr, 9, 60, &tgood, nullptr, EVERY));
    }
}
