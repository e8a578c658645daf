// batch_bind.h - how the caller's arrays of one batch reach a launch (host only, no HIP; abi.cpp, tests/cxx/batch_bind_check.cpp): the
// state rows and the DevBatch members they feed, the DevBatch of one launch request, slices and shards of a batch, trajectory blocks.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../include/nyx_hip.h"
#include "devcfg.h"

// The 13 double rows of nyx_hip_states_t in header order, and the DevBatch members a launch reads them from / writes them to.
// The first six are the Cartesian state, the first nine what the ensemble moments and the covariance mapping read.
struct StateRow { double *nyx_hip_states_t::*s; const double *DevBatch::*in; double *DevBatch::*out; };
constexpr int kStateRows = 13, kCartRows = 6, kMomentRows = 9;
#define NYX_ROW(s, b) {&nyx_hip_states_t::s, &DevBatch::b, &DevBatch::o_##b}
constexpr StateRow kStateRow[kStateRows] = {NYX_ROW(x_km, x), NYX_ROW(y_km, y), NYX_ROW(z_km, z), NYX_ROW(vx_km_s, vx), NYX_ROW(vy_km_s, vy),
                                            NYX_ROW(vz_km_s, vz), NYX_ROW(cr, cr), NYX_ROW(cd, cd), NYX_ROW(prop_mass_kg, mprop),
                                            NYX_ROW(dry_mass_kg, mdry), NYX_ROW(extra_mass_kg, mextra), NYX_ROW(srp_area_m2, asrp),
                                            NYX_ROW(drag_area_m2, adrag)};
#undef NYX_ROW

// The six state rows of nyx_hip_traj_t (DevBatch.t_state), in the same order.
constexpr double *nyx_hip_traj_t::*kTrajRow[kCartRows] = {&nyx_hip_traj_t::x_km, &nyx_hip_traj_t::y_km, &nyx_hip_traj_t::z_km,
                                                          &nyx_hip_traj_t::vx_km_s, &nyx_hip_traj_t::vy_km_s, &nyx_hip_traj_t::vz_km_s};

// What one launch of a context is asked for.  bind_batch reads the batch part; launch() (abi.cpp) the stream and the two switches.
struct LaunchReq {
    const nyx_hip_states_t *in = nullptr;
    nyx_hip_states_t *out = nullptr;
    nyx_hip_step_stats_t *stats = nullptr;  // (optional)
    int64_t duration_ns = 0, end_epoch_ns = 0;
    bool use_end = false;                   // run until end_epoch_ns, not for duration_ns
    const nyx_hip_traj_t *traj = nullptr;   // dense output (optional; capacity 0 = none)
    const int64_t *dur_ns = nullptr;        // per-trajectory durations (covariance-mapping segments), overriding duration_ns
    const DevBatch *ev = nullptr;           // stop condition: only its ev_* fields are read
    void *stream = nullptr;                 // hipStream_t
    bool timed = false, calibrating = false;  // record the kernel's time (nyx_hip_last_kernel_ms); one of calibrate()'s launches
};

// A launch's DevBatch as far as the request's arrays go; the context adds its own allocations (cooperative mailboxes, prof, stm_hist).
// `stm`: the context carries STMs; `pred`: the device copy of a fused covariance-mapping loop's arguments, or null.  rc: a refusal.
struct BoundBatch { DevBatch bt; int rc = NYX_HIP_RC_OK; const char *error = nullptr; };
inline BoundBatch bind_batch(const LaunchReq &r, bool stm, const struct PredictArgs *pred) {
    BoundBatch b;
    DevBatch &bt = b.bt;
    std::memset(&bt, 0, sizeof bt);
    const nyx_hip_states_t &in = *r.in, &out = *r.out;
    bt.n = in.n;
    bt.duration_ns = r.duration_ns; bt.end_epoch_ns = r.end_epoch_ns; bt.use_end_epoch = r.use_end ? 1 : 0;
    bt.epoch_ns = in.epoch_ns; bt.step_in = in.step_ns;
    bt.o_epoch_ns = out.epoch_ns; bt.o_step = out.step_ns;
    for (const StateRow &row : kStateRow) { bt.*row.in = in.*row.s; bt.*row.out = out.*row.s; }
    bt.dur_ns = r.dur_ns; bt.pred = pred;
    if (r.ev) {
        bt.ev_on = 1; bt.ev = r.ev->ev; bt.ev_mu = r.ev->ev_mu;
        bt.ev_prev = r.ev->ev_prev; bt.ev_count = r.ev->ev_count; bt.ev_found = r.ev->ev_found;
    }
    if (stm) {
        if (!in.stm || !out.stm) { b.rc = NYX_HIP_RC_BAD_ARG; b.error = "STM context: in->stm and out->stm are mandatory"; return b; }
        bt.stm = in.stm; bt.o_stm = out.stm;
    }
    if (r.traj && r.traj->capacity > 0) {
        const nyx_hip_traj_t &t = *r.traj;
        bt.traj_cap = t.capacity; bt.t_epoch = t.epoch_ns; bt.t_len = t.len;
        bool all = t.epoch_ns && t.len;
        for (int c = 0; c < kCartRows; ++c) all = (bt.t_state[c] = t.*kTrajRow[c]) && all;
        if (!all) { b.rc = NYX_HIP_RC_BAD_ARG; b.error = "traj: every array is mandatory"; return b; }
    }
    if (const nyx_hip_step_stats_t *st = r.stats) {
        bt.status = st->status; bt.last_step_ns = st->last_step_ns; bt.last_error = st->last_error;
        bt.last_attempts = st->last_attempts; bt.n_acc = st->n_accepted; bt.n_rej = st->n_rejected; bt.n_evals = st->n_evals;
    }
    return b;
}

// Trajectories [lo, lo + n) of a batch: every array offset (null ones stay null), the STMs by 81 doubles per trajectory.
inline nyx_hip_states_t states_at(const nyx_hip_states_t &s, int64_t lo, int64_t n) {
    nyx_hip_states_t v = s;
    v.n = n;
    v.epoch_ns = s.epoch_ns ? s.epoch_ns + lo : nullptr;
    for (const StateRow &row : kStateRow) v.*row.s = s.*row.s ? s.*row.s + lo : nullptr;
    v.stm = s.stm ? s.stm + lo * 81 : nullptr;
    v.step_ns = s.step_ns ? s.step_ns + lo : nullptr;
    return v;
}
inline nyx_hip_step_stats_t stats_at(const nyx_hip_step_stats_t &s, int64_t lo) {
    nyx_hip_step_stats_t v = s;
    auto off = [&](auto *p) { return p ? p + lo : p; };
    v.status = off(s.status); v.last_step_ns = off(s.last_step_ns); v.last_error = off(s.last_error);
    v.last_attempts = off(s.last_attempts); v.n_accepted = off(s.n_accepted); v.n_rejected = off(s.n_rejected); v.n_evals = off(s.n_evals);
    return v;
}

// Shard k of m of an n-trajectory batch (nyx_hip_propagate_batch_sharded) starts at n k / m and ends where shard k + 1 starts.
// (nyx_amd.mc.shard_bounds cuts otherwise: divmod, the larger shards first.)
inline int64_t shard_begin(int64_t n, int64_t k, int64_t m) { return n * k / m; }

// One trajectory block of `capacity` states of n trajectories: the epochs, the six state rows (step-major, capacity * n slots
// each), then len[n].  The epochs and the rows are given one slot each at least (a block of capacity 0 still holds len).
inline size_t traj_block_bytes(int64_t capacity, int64_t n) { return std::max<size_t>((size_t)capacity * (size_t)n, 1) * 7 * sizeof(double) + (size_t)n * sizeof(int32_t); }
inline nyx_hip_traj_t traj_in_block(void *block, int64_t capacity, int64_t n) {
    const size_t slots = (size_t)capacity * (size_t)n, slots1 = std::max<size_t>(slots, 1);
    nyx_hip_traj_t t;
    std::memset(&t, 0, sizeof t);
    t.capacity = capacity;
    t.epoch_ns = (int64_t *)block;
    double *base = (double *)block + slots1;
    for (int c = 0; c < kCartRows; ++c) t.*kTrajRow[c] = base + (size_t)c * slots;
    t.len = (int32_t *)(base + 6 * slots1);
    return t;
}

// Dense output of the shard [lo, lo + m) (step-major, stride m) into the batch's arrays (stride n), capacity states each.
inline void scatter_traj(const nyx_hip_traj_t &shard, int64_t lo, int64_t m, const nyx_hip_traj_t &batch, int64_t n) {
    std::memcpy(batch.len + lo, shard.len, (size_t)m * sizeof(int32_t));
    for (int64_t s = 0; s < batch.capacity; ++s) {
        std::memcpy(batch.epoch_ns + s * n + lo, shard.epoch_ns + s * m, (size_t)m * sizeof(int64_t));
        for (int c = 0; c < kCartRows; ++c) std::memcpy(batch.*kTrajRow[c] + s * n + lo, shard.*kTrajRow[c] + s * m, (size_t)m * sizeof(double));
    }
}
