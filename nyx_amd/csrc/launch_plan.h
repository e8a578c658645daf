// launch_plan.h - launch policy of a propagation context (host only; abi.cpp, tests/cxx/launch_plan_check.cpp): the waves per
// workgroup and the STM layout, the role of every wave, the harmonics columns every wave walks, and whether helper workgroups run
// and how many.  The column schedules fix the summation order, hence every bit of a result.
//
// Pure functions of their arguments: the DevCfg they plan into (its force-model part is read, its schedule part written), the
// PlanInputs below, and the SchedShape the schedules in that DevCfg were built for.  No device, no HIP.
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <map>
#include <tuple>
#include <vector>

#include "devcfg.h"
#include "col_partition.h"

// Per-wave column weights, calibrated on the device for every workgroup shape a context has launched (abi.cpp, calibrate()):
// key = (waves per workgroup, pipelined loop, quad layout, cooperative share in tenths or -1 when working alone);
// value [0..16): speed weights, [16..32): measured duties (harmonics-term units).
typedef std::tuple<int, int, int, int> WKey;
typedef std::map<WKey, std::array<double, 2 * DEV_MAX_WAVES>> WeightMap;

// Everything the planner reads besides the DevCfg.
struct PlanInputs {
    const nyx_hip_tuning_t &tune;
    const std::vector<int32_t> &col_len;  // rows per column (index = c)
    const double *role_handicap;          // [3] integrator, almanac, perturbations (harmonics-term units)
    int terms2;                           // table rows of the second gravity field
    int ed_reuse_fit;                     // fields of stage-0 epoch data an unchained pipelined loop may carry between attempts (LDS room)
    int n_cu;                             // CUs of the device (0: unknown)
    int forced_waves;                     // nyx_hip_ctx_set_column_waves (0: by configuration)
    int forced_quad;                      // STM layout: -1 = by ensemble size, 0 = 64 trajectories x D3 per workgroup, 1 = quad layout
    const WeightMap &weights;
};

// What the schedules in a DevCfg were built for.  Output of one plan and input of the next: a launch rebuilds the schedules only
// when its shape differs from this one.
struct SchedShape {
    bool quad = false;     // the STM quad layout
    int coop_parts = 1;    // sub-jobs per evaluation (1, or 2: two helper workgroups per owner and evaluation; fan-out: 2 .. DEV_FAN_MAX)
    bool coop_fan = false; // the fan-out mode: coop_parts DEDICATED helper workgroups per owner (small shards, see plan_cooperation)
};

// The cooperative mode of one launch (plan_cooperation).
struct CoopPlan {
    bool run = false;      // helper workgroups run beside the owners
    int64_t n_own = 0;     // trajectory-owning workgroups
    int64_t base = 0;      // block index of the first helper
    int parts = 1;         // sub-jobs per evaluation
    bool fan = false;      // the fan-out mode
    int64_t helpers = 0;
    double coop_frac = 0.0;  // share of the harmonics terms the helpers take (DevCfg.coop_frac)
    int64_t boxes = 0;       // mailboxes the launch touches: one per owner
    int64_t answers = 0;     // answer blocks behind the scan words: one per (owner, part) beyond part 0 (fan-out), one per owner (two parts)
};

// The column weights' key of a workgroup shape (WeightMap).
inline WKey weight_key(const DevCfg &dc, int n_waves, bool quad, bool coop) {
    return WKey(n_waves, (dc.pipe && (!(dc.flags & NYX_HIP_FLAG_STM) || quad)) ? 1 : 0, quad ? 1 : 0, coop ? (int)(dc.coop_frac * 10.0 + 0.5) : -1);
}

inline bool has_nonzero(const double *v, int n) { for (int k = 0; k < n; ++k) if (v[k] != 0.0) return true; return false; }

// hc[w] of a wave that walks no columns at all: the integrator wave of a workgroup of eight or more waves that is pipelined or has no
// role duties stated by the caller (build_schedule: n_waves >= 8 && (pipe || no tuning.role_duties)).  A duty, not a number: the
// water-filling's bracket caps every duty at kDutyBracketCap, and a measured duty never replaces it.
constexpr double kNoColumns = 1e9;
constexpr double kDutyBracketCap = 1e6;
inline bool walks_no_columns(double hc) { return hc >= 1e8; }

// wave w of `sd` walks the columns cols[0..n) (ascending, possibly with gaps): one range per contiguous run.  False if that takes
// more than DEV_MAX_RANGES ranges.
inline bool set_ranges(DevSched &sd, int w, const int *cols, size_t n) {
    int nr = 0;
    for (size_t a = 0; a < n;) {
        size_t e = a + 1;
        while (e < n && cols[e] == cols[e - 1] + 1) ++e;
        if (nr >= DEV_MAX_RANGES) return false;
        sd.range_c0[w][nr] = cols[a]; sd.range_cnt[w][nr] = (int)(e - a); ++nr;
        a = e;
    }
    sd.n_ranges[w] = nr;
    return true;
}

// Column schedule: wave w walks at most two contiguous ranges — long columns from the low-c end,
// topped up with short columns from the high-c end — so that one complex power per range suffices.
// Waves 0/1/2 also carry the integrator / almanac / perturbation duties (`role_handicap`, in units of
// one harmonics term), so they receive a reduced share of the columns, possibly none.
// Water-filling of the columns [c_lo, c_hi] over `n_waves` waves with per-wave handicaps hc[] (work a wave does besides
// its columns, in harmonics-term units) and SIMD age weights.  Wave 0 takes what is left.
// `list`: the columns to distribute, ascending (= longest first).  Returns false if a wave would need more than
// DEV_MAX_RANGES contiguous ranges.
inline bool fill_schedule(const PlanInputs &in, const DevCfg &dc, bool quad, DevSched &sd, int n_waves, const std::vector<int> &list,
                          const double *hc_model, bool all_columns) {
    double hc[DEV_MAX_WAVES];
    for (int w = 0; w < DEV_MAX_WAVES; ++w) hc[w] = hc_model[w];
    for (int w = 0; w < DEV_MAX_WAVES; ++w) sd.n_ranges[w] = 0;
    if (list.empty()) return true;
    // (debug_flags 0x8000: the two-ended column fill of rounds 1-3 everywhere; 0x10000: contiguous runs whatever the feed - the A/B
    //  partner of the streamed walk; 0x2000000: the linear partition of round 4 for the cooperative 70x70 shape too)
    const bool block_schedule = (in.tune.debug_flags & 0x8000) == 0;   // one contiguous run of columns per wave where the owner streams the table
    const bool block_force = (in.tune.debug_flags & 0x10000) != 0;
    const bool fit_partition = (in.tune.debug_flags & 0x2000000) == 0;  // ... placed along the column list in a free wave order (below)
    // cost of a column in rows: its length plus what it costs to START one (header, complex power of the range, a cold first batch).
    // With the short columns of a small field in the quad layout that start is most of a column: 21x21, 1 000 trajectories, sixty
    // segments: 11.45 ms with 0 rows, 11.1 with 4, 10.83 with 6, 10.95 with 8 (four runs each, +-0.03).  70x70 plain kernel: no effect
    // up to 6, slower beyond (the measured per-wave weights already carry it there).  Round 4, with the roles fanned out over eight of
    // the sixteen waves: 6 rows left the oldest pure column wave without a column (the two-ended fill ran out of columns before it
    // reached wave 4) and the youngest ones with the longest; config 4, three runs each: 10.10 ms with 6, 9.83 with 8, 9.55-9.60 with
    // 9 ... 18 (a plateau: every wave holds one or two columns then) - same bits, the quad layout's sums do not depend on the split.
    double col_fix = (quad && n_waves == DEV_MAX_WAVES) ? 12.0 : 0.0;  // (the quad layout's production shape: sixteen waves)
    if (in.tune.column_start_cost >= 0.0) col_fix = in.tune.column_start_cost;
    auto cost = [&](int c) { return (double)in.col_len[c] + col_fix; };
    double terms = 0.0;
    for (int c : list) terms += cost(c);
    // Per-wave weights.  The four waves that share a SIMD (w, w+4, w+8, w+12) are arbitrated oldest-first, so with equal
    // shares the oldest finishes early and the youngest runs the tail alone, with nothing to hide its scalar-load latency;
    // role waves carry their duty besides.  The weights are MEASURED: calibrate() runs the workload's own first steps with
    // the in-kernel cycle accounting and moves columns from the late waves to the early ones until the windows agree;
    // before that (and with calibration off) a structural guess by age class is used.
    double per_wave[DEV_MAX_WAVES];
    const bool blk = block_schedule && n_waves == DEV_MAX_WAVES && !quad && ((dc.harm_feed & 1) || block_force);
    // (the runs of a block schedule placed along the list in a free wave order: the cooperative 70x70 shape, see below)
    const bool fit = blk && !all_columns && dc.n_cols <= 96 && fit_partition;
    {
        const auto it = in.weights.find(weight_key(dc, n_waves, quad, !all_columns));
        // The cost model of NYX_HIP_SCHED_MODEL: the speed of a wave is a property of its place in the workgroup (the four waves of a
        // SIMD are arbitrated oldest first; role waves and their SIMD-mates run differently) and of the workgroup's shape, not of
        // the force model.  Measured once with the calibration below on the BASELINE workloads (tools/dump_weights.py, two contexts
        // each, agreement ~2 %) and frozen here, so that the default schedule - hence the summation order, hence every bit of the
        // result - is the same in every context, process and rank.
        static const double model_coop[16] = {1.70, 1.66, 1.48, 2.14, 2.08, 1.70, 1.65, 1.67, 1.45, 0.97, 1.05, 1.02, 0.70, 0.53, 0.56, 0.55};
        static const double model_solo[16] = {1.41, 1.41, 1.26, 1.61, 1.59, 1.29, 1.375, 1.23, 1.06, 0.98, 0.98, 0.98, 0.77, 0.69, 0.70, 0.70};
        // (quad table, round 5: re-fitted by hill-climbing the explicit weights on config 4 with the position-only pieces of phase C on
        //  the DCM wave (assign_roles, DEV_ROLE_QPRE) - with the integrator's window shorter the column waves are the period again:
        //  8.99 ms with the round-4 table {0.70 x 4, 1.26, 2.03, 1.78, 1.59, 1.58, 1.68, 0.96, 1.02, 0.875, 0.93, 0.86, 0.91}, 8.61 with this)
        static const double model_quad[16] = {0.700, 0.700, 0.505, 0.876, 1.173, 1.490, 1.795, 2.380, 3.445, 2.528, 0.927, 1.020, 0.875, 0.930, 0.941, 1.124};
        // Round 4, the shapes that deal ONE contiguous run of columns per wave (below) and stream the table in the trajectory-owning
        // workgroups: fitted with tools/tune_schedule.py (windows of every wave -> rows that would equalise them -> weights, best
        // kernel time of 8-14 iterations, two boxes) on configs[1] at 10 000 (cooperative) and 16 384 trajectories (alone) and on
        // configs[4] (150x150, cooperative, helper jobs of several columns).  The role duties of the water-filling are unchanged.
        // (cooperative 70x70 table: fitted on the FULL day of configs[1] - the perturbation wave's duty grows over the day, 14 k -> 20 k cycles
        //  per evaluation once the lanes' eclipse transitions no longer coincide, and a table fitted on the first three hours overloaded it:
        //  719 -> 680 ms per 10 000 x 24 h, same box)
        static const double model_coop_blk[16] = {1.00, 1.413, 0.549, 1.946, 1.892, 1.523, 1.588, 1.292, 1.066, 0.828, 0.937, 0.692, 0.430, 0.347, 0.357, 0.142};
        static const double model_coop_big_blk[16] = {1.00, 1.755, 1.706, 1.802, 1.733, 1.22, 1.246, 1.181, 1.087, 0.672, 0.621, 0.604, 0.549, 0.279, 0.284, 0.255};
        static const double model_solo_blk[16] = {1.00, 1.612, 1.263, 1.906, 1.764, 1.346, 1.331, 1.198, 1.113, 0.757, 0.659, 0.568, 0.513, 0.398, 0.291, 0.27};
        // Round 5, the cooperative 70x70 shape with its runs placed in a free wave order (`fit`, below): the column waves' weights as
        // tools/tune_schedule.py settles on them with that partition (full day of configs[1]; the role waves keep the table's values -
        // every row more on them costs the integrator's chain: 614 ms with these, 662 with ten rows more on each of the two).
        // Same box, product kernel, 24 h: 625.0 ms linear partition, 617.0 free order with the old table, 614.0 with this one.
        static const double model_coop_fit[16] = {1.00, 1.413, 0.549, 1.95, 1.83, 1.48, 1.40, 1.23, 1.04, 0.88, 0.85, 0.62, 0.50, 0.36, 0.34, 0.16};
        const double *model = quad ? model_quad
                              : (blk ? (all_columns ? model_solo_blk : (dc.n_cols > 96 ? model_coop_big_blk : (fit ? model_coop_fit : model_coop_blk)))
                                     : (all_columns ? model_solo : model_coop));
        for (int w = 0; w < DEV_MAX_WAVES; ++w)
            per_wave[w] = it != in.weights.end() ? it->second[w] : (n_waves == 16 ? model[w] : 1.0);
        if (it != in.weights.end())  // measured duties replace the model's (the integrator keeps its window free: hc_model[0])
            for (int w = 0; w < n_waves; ++w)
                if (!walks_no_columns(hc_model[w])) hc[w] = it->second[DEV_MAX_WAVES + w];
    }
    if (in.tune.schedule == NYX_HIP_SCHED_EXPLICIT) {  // explicit weights: per wave, or one per SIMD age class
        const bool per = has_nonzero(in.tune.wave_weights, 16), age_on = has_nonzero(in.tune.age_weights, 4);
        for (int w = 0; w < DEV_MAX_WAVES; ++w) {
            if (per) per_wave[w] = in.tune.wave_weights[w];
            else if (age_on && n_waves == 16) per_wave[w] = in.tune.age_weights[w / 4];
        }
    }
    auto wgt = [&](int w) { return per_wave[w]; };
    // water-filling: level such that sum_w max(0, level * weight_w - hc[w]) = terms
    double level = 0.0;
    {
        double hsum = 0.0;
        for (int w = 0; w < n_waves; ++w) hsum += std::min(hc[w], kDutyBracketCap);
        double lo = 0.0, hi = 4.0 * (terms + hsum);
        for (int it = 0; it < 80; ++it) {
            level = 0.5 * (lo + hi);
            double sum = 0.0;
            for (int w = 0; w < n_waves; ++w) sum += std::max(0.0, level * wgt(w) - hc[w]);
            if (sum < terms) lo = level; else hi = level;
        }
    }
    auto target = [&](int w) { return std::max(0.0, level * wgt(w) - hc[w]); };
    if (blk) {
        // ONE contiguous run of columns per wave (the hybrid stream walks a run as one piece of the table: every range START costs it a
        // pipeline fill, the complex power of the range and up to seven rows in front of the run - with two or three ranges per wave
        // and evaluation that is a third of a 70x70 owner's work).  Linear partition of the list (longest columns first) at the
        // cumulative targets; the waves with the largest targets take the long columns, role waves the short ones at the end, where
        // the granularity is finest.  The integrator wave (target 0 in the pipelined loop) gets nothing.
        std::vector<int> order;
        for (int w = 0; w < n_waves; ++w) order.push_back(w);
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return target(a) > target(b); });
        if (fit) {
            // Round 5, the same contiguous runs in a FREE wave order.  The linear partition above deals whole columns at the cumulative
            // targets in descending target order, so a wave's load is off by up to half a column - +-25 rows of ~230 for the waves
            // that hold the 50-row columns of a 70x70 owner, and a column wave is bound by its OWN issue rate (one VALU instruction per
            // ~9 cycles and wave, tools/_exp/exec_rate.hip): the two or three waves rounded UP set the workgroup's period.  A run of j
            // columns starting at length L sums to jL - j(j-1)/2: which sums exist depends on WHERE in the list a run sits, so the
            // waves are placed along the list in whatever order lets every one of them meet its target - a depth-first search over
            // (columns consumed, waves placed) for the smallest tolerance D with |load_w - target_w| <= D * weight_w for every wave
            // (the weight is the wave's speed: the same TIME error everywhere; col_partition.h).  A pure function of the configuration, like the rest.
            std::vector<int> act;
            for (int w : order) if (target(w) > 0.0) act.push_back(w);
            std::vector<double> cst, tg, wg;
            for (int c : list) cst.push_back(cost(c));
            for (int w : act) { tg.push_back(target(w)); wg.push_back(wgt(w)); }
            std::vector<int> seq_w, seq_k;   // the placement found: wave index (into act) and its first column, in list order
            if (nyx_place_runs(cst, tg, wg, seq_w, seq_k)) {
                for (size_t q = 0; q < seq_w.size(); ++q) {
                    const size_t k0 = (size_t)seq_k[q], k1 = q + 1 < seq_w.size() ? (size_t)seq_k[q + 1] : list.size();
                    if (!set_ranges(sd, act[seq_w[q]], list.data() + k0, k1 - k0)) return false;
                }
                return true;
            }
            // (no placement within the widest tolerance: the linear partition below)
        }
        double cum_t = 0.0, cum_r = 0.0;
        size_t k = 0;
        for (size_t q = 0; q < order.size(); ++q) {
            const int w = order[q];
            cum_t += target(w);
            const size_t k0 = k;
            const bool last = q + 1 == order.size() || target(order[q + 1]) <= 0.0;
            while (k < list.size() && (last || cum_r + 0.5 * cost(list[k]) <= cum_t)) { cum_r += cost(list[k]); ++k; }
            // (the list is ascending in column number but may have gaps - the helper's columns: a run is split at every gap)
            if (!set_ranges(sd, w, list.data() + k0, k - k0)) return false;
            if (last) break;
        }
        return true;
    }
    int lo = 0, hi = (int)list.size() - 1;  // indices into `list`
    // plain column workers first (highest wave index), role waves last so they take what is left
    // (round 6: what is left goes to the last wave that WALKS columns - the integrator wave of a pipelined workgroup walks none, and a
    //  list of two or three short columns, the owner's share in the fan-out mode of a field below degree 40, is all "left over":
    //  dealt to wave 0 it was never evaluated - 59 m after two hours, tests/test_gpu_rotation.py)
    const int last_w = (walks_no_columns(hc[0]) && n_waves > 1) ? 1 : 0;
    for (int w = n_waves - 1; w >= last_w; --w) {
        const double tgt = target(w);
        std::vector<int> mine;
        if (w == last_w) {
            for (int k = lo; k <= hi; ++k) mine.push_back(list[k]);
            lo = hi + 1;
        } else {
            double load = 0.0;
            while (lo <= hi && load + 0.5 * cost(list[lo]) <= tgt) { load += cost(list[lo]); mine.push_back(list[lo++]); }
            std::vector<int> tail;
            while (lo <= hi && load + 0.5 * cost(list[hi]) <= tgt) { load += cost(list[hi]); tail.push_back(list[hi--]); }
            mine.insert(mine.end(), tail.rbegin(), tail.rend());
        }
        if (!set_ranges(sd, w, mine.data(), mine.size())) return false;
    }
    return true;
}

// Role fan-out (small ensembles: the STM quad layout, and dynamics without a gravity field): with few workgroups on the
// chip what counts is the latency of ONE force evaluation, and the almanac and perturbation duties are its longest serial
// pieces.  They are dealt over several waves - the DCM and the body slots (or the distinct ephemeris segments, fanout_almanac_units) over up to DEV_MAX_ALM almanac waves (longest
// first), point masses (+ tides) and SRP (+ drag) over two perturbation waves - each writing its own LDS rows, so the
// arithmetic and its order do not change.  Costs in harmonics-term units, as `role_handicap`.
// Units of the almanac duty: the DCM, then either the DISTINCT ephemeris segments of all chains (segment mode: Earth -> EMB sits on
// every chain of an Earth-centred run and is evaluated once; the readers sum the chains, ed_bp() in the kernel) when their vectors
// fit the body rows of the epoch data - 4 with a DCM, 7 without - or the body slots.
inline int distinct_segments(const DevCfg &dc, int *useg_seg = nullptr) {
    int n = 0, list[DEV_MAX_SEG];
    for (int s = 0; s < dc.n_slots; ++s)
        for (int k = 0; k < dc.slot[s].n_chain; ++k) {
            bool seen = false;
            for (int q = 0; q < n; ++q) seen = seen || list[q] == dc.slot[s].seg[k];
            if (!seen && n < DEV_MAX_SEG) list[n++] = dc.slot[s].seg[k];
        }
    if (useg_seg) for (int q = 0; q < n; ++q) useg_seg[q] = list[q];
    return n;
}
inline bool segment_units_fit(const DevCfg &dc) {
    const bool dcm = dc.has_grav || dc.has_drag || dc.has_tides;
    const int nu = distinct_segments(dc);
    return nu >= 2 && nu <= (dcm ? DEV_MAX_SLOTS : DEV_MAX_SLOTS + 3);
}
// the almanac waves evaluate distinct segments: tell the kernel where their vectors live
inline void use_segment_units(DevCfg &dc) {
    dc.seg_mode = 1;
    dc.n_useg = distinct_segments(dc, dc.useg_seg);
    dc.ed_seg_base = (dc.has_grav || dc.has_drag || dc.has_tides) ? 9 : 0;
    for (int sl = 0; sl < dc.n_slots; ++sl)
        for (int k = 0; k < dc.slot[sl].n_chain; ++k)
            for (int u = 0; u < dc.n_useg; ++u)
                if (dc.useg_seg[u] == dc.slot[sl].seg[k]) dc.slot[sl].useg[k] = u;
}
inline int fanout_almanac_units(const DevCfg &dc, int *unit_mask, double *unit_cost) {
    int n = 0;
    if (dc.has_grav || dc.has_drag || dc.has_tides) { unit_mask[n] = DEV_ROLE_DCM; unit_cost[n] = 18.0; ++n; }
    if (segment_units_fit(dc)) {
        int us[DEV_MAX_SEG];
        const int nu = distinct_segments(dc, us);
        for (int u = 0; u < nu; ++u) { unit_mask[n] = 1 << u; unit_cost[n] = 3.0 + 0.75 * dc.seg[us[u]].n_coef; ++n; }
        return n;
    }
    for (int s = 0; s < dc.n_slots; ++s) { unit_mask[n] = 1 << s; unit_cost[n] = 12.0 * dc.slot[s].n_chain; ++n; }
    return n;
}
inline bool want_fanout(const PlanInputs &in, const DevCfg &dc, bool quad) {
    if (in.tune.role_fanout >= 0) return in.tune.role_fanout != 0;
    return quad || !dc.has_grav;
}
inline int fanout_role_waves(const DevCfg &dc, int *n_alm_out = nullptr, int *n_pert_out = nullptr) {
    int um[10]; double uc[10];
    const int units = fanout_almanac_units(dc, um, uc);
    const int n_alm = std::min(DEV_MAX_ALM, std::max(units, 0));
    const int n_pert = ((dc.n_pm > 0 || dc.has_tides || dc.has_grav2) ? 1 : 0) + ((dc.has_srp || dc.has_drag) ? 1 : 0);
    if (n_alm_out) *n_alm_out = n_alm;
    if (n_pert_out) *n_pert_out = n_pert;
    return 1 + n_alm + n_pert;
}

// Deals the roles of an n_waves workgroup (DevCfg.role_*) and returns the serial duty of every wave in `hc`.
inline void assign_roles(const PlanInputs &in, DevCfg &dc, bool quad, int n_waves, bool fanout, double *hc) {
    const int all_alm = DEV_ROLE_DCM | ((1 << dc.n_slots) - 1);
    const int all_pert = (DEV_PERT_PM | DEV_PERT_SRP) << 16;
    for (int w = 0; w < DEV_MAX_WAVES; ++w) { dc.role_kind[w] = DEV_ROLE_COLUMNS; dc.role_mask[w] = 0; dc.role_slot[w] = 0; hc[w] = 0.0; }
    dc.n_alm = 1;
    dc.seg_mode = 0;
    dc.offload = 0;
    dc.qpre_off = 0;
    const double *rh = in.role_handicap;
    if (n_waves == 1) { dc.role_kind[0] = DEV_ROLE_ALL; dc.role_mask[0] = all_alm | all_pert; hc[0] = rh[0] + rh[1] + rh[2]; return; }
    dc.role_kind[0] = DEV_ROLE_INTEG; hc[0] = rh[0];
    if (n_waves == 2 || dc.merge_roles) { dc.role_kind[1] = DEV_ROLE_ALMANAC_PERT; dc.role_mask[1] = all_alm | all_pert; hc[1] = rh[1] + rh[2]; return; }
    int n_alm = 1, n_pert = 1;
    if (fanout && fanout_role_waves(dc, &n_alm, &n_pert) <= n_waves && n_alm >= 1 && n_pert >= 1) {
        const bool stm = (dc.flags & NYX_HIP_FLAG_STM) != 0;
        // the duties: almanac shares (longest unit first onto the least loaded share), then the perturbation shares
        struct Duty { int kind, mask, slot; double cost; };
        std::vector<Duty> duties;
        {
            int um[10]; double uc[10];
            const int units = fanout_almanac_units(dc, um, uc);
            int order[10];
            for (int k = 0; k < units; ++k) order[k] = k;
            std::sort(order, order + units, [&](int a, int b) { return uc[a] > uc[b]; });
            double load[DEV_MAX_ALM] = {0.0};
            int amask[DEV_MAX_ALM] = {0};
            for (int k = 0; k < units; ++k) {
                int best = 0;
                for (int a = 1; a < n_alm; ++a) if (load[a] < load[best]) best = a;
                amask[best] |= um[order[k]];
                load[best] += uc[order[k]];
            }
            for (int a = 0; a < n_alm; ++a) duties.push_back({DEV_ROLE_ALMANAC, amask[a], a, load[a]});
            dc.n_alm = n_alm;
        }
        // (measured on the device, in units of ~250 cycles: a plain point mass 4, a dual one 11; SRP with its occultation 12 + 8 per
        //  shadow body, dual 25 + 25; drag 10; tides 14 + 8 per perturber)
        const double pm_cost = (stm ? 11.0 : 4.0) * dc.n_pm + (dc.has_tides ? (stm ? 3.0 : 1.0) * (14.0 + 8.0 * dc.t_n) : 0.0) +
                               (dc.has_grav2 ? 8.0 + 0.2 * in.terms2 : 0.0);
        const double srp_cost = (dc.has_srp ? (stm ? 25.0 + 25.0 * dc.n_shadow : 12.0 + 8.0 * dc.n_shadow) : 0.0) + (dc.has_drag ? 10.0 : 0.0);
        if (n_pert == 2) {
            duties.push_back({DEV_ROLE_PERT, DEV_PERT_PM << 16, 0, pm_cost});
            duties.push_back({DEV_ROLE_PERT, DEV_PERT_SRP << 16, 0, srp_cost});
        } else {
            duties.push_back({DEV_ROLE_PERT, all_pert, 0, pm_cost + srp_cost});
        }
        // Placement: wave w runs on SIMD w % 4, and a force evaluation is bound by the busiest SIMD's role work (the role code
        // is VALU-heavy: sincos, Chebyshev chains, divisions).  Heaviest duty first onto the least loaded SIMD; the integrator
        // (wave 0, ~50 units with its phases A and C) sits on SIMD 0.
        double simd_load[4] = {stm ? 52.0 : 26.0, 0.0, 0.0, 0.0};
        bool taken[DEV_MAX_WAVES] = {true};
        std::sort(duties.begin(), duties.end(), [](const Duty &a, const Duty &b) { return a.cost > b.cost; });
        bool placed_all = true;
        for (const Duty &d : duties) {
            int best_w = -1;
            double best_load = 1e300;
            for (int sd = 0; sd < 4; ++sd) {
                int w = -1;
                for (int k = sd; k < n_waves; k += 4) if (!taken[k]) { w = k; break; }
                if (w >= 0 && simd_load[sd] < best_load) { best_load = simd_load[sd]; best_w = w; }
            }
            if (best_w < 0) { placed_all = false; break; }
            taken[best_w] = true;
            simd_load[best_w % 4] += d.cost;
            dc.role_kind[best_w] = d.kind; dc.role_mask[best_w] = d.mask; dc.role_slot[best_w] = d.slot; hc[best_w] = d.cost;
        }
        if (placed_all) {
            if (dc.pipe && !dc.has_grav && !stm && (in.tune.debug_flags & 0x800)) {  // (0x800: A/B switch, same results)
                // pipelined, no column waves: the two lightest almanac shares take the two-body term and the head of the stage sums off
                // the integrator wave (DevCfg.offload).  Rounds 3-4 default; OFF since round 5: the integrator's publish-first window
                // (role_loop, `fastp`) is shorter than the offloaded one and the almanac SIMDs are the busiest of the workgroup
                // (config 3: 46.7 -> 44.7 ms without it, same bits)
                // (what an almanac wave has to spare depends on whom it shares its SIMD with: the integrator's SIMD last, then by the SIMD's load)
                int w1 = -1, w2 = -1;
                auto spare = [&](int w) { return (w % 4 == 0 ? 1e6 : 0.0) + simd_load[w % 4] + hc[w]; };
                for (int w = 1; w < n_waves; ++w) {
                    if (dc.role_kind[w] != DEV_ROLE_ALMANAC) continue;
                    if (w1 < 0 || spare(w) < spare(w1)) { w2 = w1; w1 = w; }
                    else if (w2 < 0 || spare(w) < spare(w2)) w2 = w;
                }
                if (w1 >= 0) {
                    if (w2 < 0) w2 = w1;
                    dc.role_mask[w1] |= DEV_ROLE_SUMS; hc[w1] += 4.0;
                    dc.role_mask[w2] |= DEV_ROLE_TWOBODY; hc[w2] += 2.0;
                    dc.offload = 1;
                }
            }
            if (stm && quad && !(in.tune.debug_flags & 0x4000000)) {  // (0x4000000: A/B switch, same results)
                // quad STM layout: the position-only pieces of phase C (quad_pre, 4-5 k cycles of the integrator's window per evaluation)
                // go to the almanac wave with the most time to spare - the integrator's chain is what bounds such a workgroup
                // (the wave that holds the DCM when there is one: in the sixteen-wave shape it walks no columns, the segment waves do)
                int wq = -1;
                for (int w = 1; w < n_waves; ++w)
                    if (dc.role_kind[w] == DEV_ROLE_ALMANAC && (dc.role_mask[w] & DEV_ROLE_DCM)) wq = w;
                if (wq < 0)
                    for (int w = 1; w < n_waves; ++w) {
                        if (dc.role_kind[w] != DEV_ROLE_ALMANAC) continue;
                        if (wq < 0 || simd_load[w % 4] + hc[w] < simd_load[wq % 4] + hc[wq]) wq = w;
                    }
                if (wq >= 0) { dc.role_mask[wq] |= DEV_ROLE_QPRE; hc[wq] += 18.0; simd_load[wq % 4] += 18.0; dc.qpre_off = 1; }
            }
            if (segment_units_fit(dc)) use_segment_units(dc);  // (the almanac shares above are distinct segments)
            return;
        }
        for (int w = 1; w < DEV_MAX_WAVES; ++w) { dc.role_kind[w] = DEV_ROLE_COLUMNS; dc.role_mask[w] = 0; dc.role_slot[w] = 0; hc[w] = 0.0; }
        dc.n_alm = 1;
    }
    dc.role_kind[1] = DEV_ROLE_ALMANAC; dc.role_mask[1] = all_alm; hc[1] = rh[1];
    dc.role_kind[2] = DEV_ROLE_PERT; dc.role_mask[2] = all_pert; hc[2] = rh[2];
    // ONE almanac wave (the sixteen-wave column shapes): distinct-segment units pay here too - Earth -> EMB sits on the chain of
    // every body of an Earth-centred run and was evaluated once per BODY per stage (five Chebyshev evaluations for Sun + Moon where
    // four segments are distinct).  The wave evaluates every distinct segment once, the readers sum the chains (ed_body(): the same
    // additions in the same order, bit-identical).
    int chain_evals = 0;
    for (int sl = 0; sl < dc.n_slots; ++sl) chain_evals += dc.slot[sl].n_chain;
    if (segment_units_fit(dc) && distinct_segments(dc) < chain_evals) {
        use_segment_units(dc);
        dc.role_mask[1] = DEV_ROLE_DCM | ((1 << dc.n_useg) - 1);
    }
}

// The balanced helper dealing (build_schedule): the speed of a helper column wave on a SIMD that hosts three of them (beside the
// producer / the answering wave), and what the start of one more column on a helper wave is charged, in rows.
constexpr double kCoopFastWeight = 4.0 / 3.0;
constexpr double kCoopStartRows = 4.0;

// Roles, stage loop and column schedules of an n_waves workgroup of the shape `shape` (quad layout, cooperative parts / fan-out) into
// `dc`.  Reads dc.coop_frac, the helper share of the claim mode.  dc.coop_ok = 1 when the PRIMARY and helper schedules are valid.
inline void build_schedule(const PlanInputs &in, DevCfg &dc, const SchedShape &shape, int n_waves) {
    const bool quad = shape.quad;
    const int nc = dc.n_cols;
    for (int k = 0; k < DEV_N_SCHED; ++k)
        for (int w = 0; w < DEV_MAX_WAVES; ++w) dc.sched[k].n_ranges[w] = 0;
    dc.n_waves = n_waves;
    if (dc.has_grav2)  // the second field: every column, for whichever wave walks it (the perturbation wave with the point-mass share)
        for (int w = 0; w < DEV_MAX_WAVES; ++w) {
            dc.sched[DEV_SCHED_SECOND].n_ranges[w] = 1;
            dc.sched[DEV_SCHED_SECOND].range_c0[w][0] = 1;
            dc.sched[DEV_SCHED_SECOND].range_cnt[w][0] = dc.n_cols2;
        }
    dc.merge_roles = (in.tune.merge_roles && n_waves >= 8) ? 1 : 0;
    // pipelined stage loop: sixteen-wave workgroups (the column waves go from one stage's harmonics into the next's), and - plain
    // kernel - any workgroup of dynamics without a gravity field that has the integrator in a wave of its own: the perturbation
    // waves need the POSITION of the next stage only, which the integrator publishes inside the window, so its phases A and C run
    // beside the almanac / perturbation duties instead of in front of them
    const bool stm_cfg = (dc.flags & NYX_HIP_FLAG_STM) != 0;
    // (not with a non-central gravity field: its inputs need the body's position of the stage, which the almanac waves write late in the window)
    dc.pipe = (!dc.merge_roles && in.tune.pipelined != 0 && !(dc.has_grav && dc.g_slot >= 0) &&
               ((n_waves == DEV_MAX_WAVES && dc.has_grav) || (!dc.has_grav && !stm_cfg && n_waves >= 2 && n_waves <= 8))) ? 1 : 0;
    // (a workgroup of more than eight waves WITHOUT a gravity field exists only when the caller forces it - nyx_hip_ctx_set_column_waves -
    //  and runs the plain loop: the pipelined integrator of the sixteen-wave kernels is compiled for the gravity-field shape, INTEG_OOL)
    // roles of this workgroup shape and their serial duties (merged roles when there are fewer than three waves)
    double hc[DEV_MAX_WAVES] = {0};
    assign_roles(in, dc, quad, n_waves, want_fanout(in, dc, quad), hc);
    // speculative stage 0 (role_loop): the pipelined plain kernel with ONE almanac wave and an even stage count (the last window
    // then leaves the buffers of stage parity 0 free for the epoch data of t + h)
    // (with a gravity field: one almanac wave; without: any fan-out, almanac and perturbation duties in waves of their own)
    dc.spec = (dc.pipe && !(dc.flags & NYX_HIP_FLAG_STM) && dc.stages % 2 == 0 &&
               (dc.has_grav ? dc.n_alm == 1 : (n_waves >= 3 && dc.role_kind[1] != DEV_ROLE_ALMANAC_PERT && (dc.n_slots > 0 || dc.has_drag || dc.has_tides))) &&
               !dc.has_grav2 &&  // (the second field's wave reads the attempt's epoch at stage 0: it would have to wait for step control)
               in.tune.chained_attempts != 0) ? 1 : 0;
    dc.ed_reuse = (dc.spec || dc.seg_mode) ? 0 : in.ed_reuse_fit;  // (chained attempts need no copy of the stage-0 epoch data: a rejected lane keeps its k_0)
    if (!dc.has_grav || nc == 0) return;
    // with enough column workers the integrator keeps its window free: its serial phases A / C gate every other wave
    // (pipelined loop: the integrator wave walks NO columns at all - role_loop skips its walk -, whatever duties the caller states:
    //  round 5 found tuning.role_duties handing it 57 rows that nobody then evaluated)
    if (n_waves >= 8 && (dc.pipe || !has_nonzero(in.tune.role_duties, 3))) hc[0] = kNoColumns;
    std::vector<int> all;
    for (int c = 1; c <= nc; ++c) all.push_back(c);
    (void)fill_schedule(in, dc, quad, dc.sched[DEV_SCHED_SOLO], n_waves, all, hc, true);
    // Cooperative mode (16-wave workgroups only).  The helper takes the LONGEST columns, at most one per column wave: its job
    // time is then one long column (~18 batches), which is within 17 % of the ideal x * terms / 16 for x <= 0.35, and the
    // owner keeps the many short columns that let it balance its fifteen waves.  (Interleaving the two sets column by
    // column was measured 10-25 % slower: the helper's waves then hold a long AND a short column each.)
    if (n_waves == DEV_MAX_WAVES && nc >= 8 && shape.coop_fan) {
        // FAN-OUT mode (plan_cooperation: the idle CUs outnumber the owners at least two to one - a shard of an ensemble, a small Monte Carlo).
        // Every owner has K = coop_parts dedicated helper workgroups (propagate_kernel.hip, helper_body under NYX_COOP_FAN); the owner's
        // period is then bounded by its integrator's chain, not by column work, so the helpers take everything but the shortest columns:
        // the K * cpp longest, dealt round-robin over the parts (every part a mix of long and short: equal jobs), one column per wave,
        // the waves of a part taken round-robin over the SIMDs (eight columns = two waves per SIMD, which finish in ~10 k cycles where
        // four per SIMD need ~17 k).  The owner keeps at least two columns (its PRIMARY schedule must not be empty).
        const int K = std::min(std::max(shape.coop_parts, 2), DEV_FAN_MAX);
        const int col_waves = DEV_MAX_WAVES - 2;
        int cpp = std::min(col_waves, (nc - 2 + K - 1) / K);
        if (in.tune.coop_max_columns > 0) cpp = std::max(1, std::min(cpp, (int)in.tune.coop_max_columns / K));
        const int n_help = std::min(nc - 2, K * cpp);
        std::vector<int> own;
        for (int c = n_help + 1; c <= nc; ++c) own.push_back(c);
        for (int k = 0; k < n_help; ++k) {
            const int part = k % K, pos = k / K;       // (ascending column number = descending length)
            const int w = 1 + pos;                      // waves 1 .. 14 sit on SIMDs 1 2 3 0 1 2 3 0 ...: any prefix is balanced
            DevSched &hs = dc.sched[DEV_SCHED_FAN0 + part];
            const int r = hs.n_ranges[w]++;
            hs.range_c0[w][r] = 1 + k; hs.range_cnt[w][r] = 1;
        }
        if (n_help > 0 && !own.empty() && fill_schedule(in, dc, quad, dc.sched[DEV_SCHED_PRIMARY], n_waves, own, hc, false)) {
            dc.coop_ok = 1;
        } else {
            dc.coop_ok = 0;
            for (int k = 0; k < DEV_N_SCHED; ++k)
                if (k == DEV_SCHED_PRIMARY || k >= DEV_SCHED_FAN0)
                    for (int w = 0; w < DEV_MAX_WAVES; ++w) dc.sched[k].n_ranges[w] = 0;
        }
    } else
    if (n_waves == DEV_MAX_WAVES && nc >= 8) {
        double terms = 0.0, given = 0.0;
        for (int c = 1; c <= nc; ++c) terms += in.col_len[c];
        std::vector<int> own, help;
        const int col_waves = DEV_MAX_WAVES - 2;  // a helper's wave 0 claims jobs, its last wave answers
        // One column per helper wave is the rule for short evaluation periods (70x70: a second column makes the job longer than the
        // owner can wait, 302 ms against 182 ms).  A large field turns that around: at 150x150 the owner's period is 140 k cycles,
        // a job of one 150-row column 34 k + the hand-off, and fourteen columns are 18 % of the terms where the helpers could take
        // half - so when the one-column rule leaves the helpers below HALF of their share, their waves take up to
        // DEV_MAX_RANGES columns each (config 5: 12.05 s with 14 columns, 11.36 s with 21, 10.31 s with 28).
        int max_cols = col_waves;
        // Two-part hand-off (coop_parts == 2, chosen by plan_cooperation when the idle CUs outnumber the owners and the helpers' jobs hold
        // several columns per wave): the helpers' columns are dealt alternately into two sub-jobs that two DIFFERENT helper workgroups
        // claim - half the job per helper, so the turnaround the owner waits for halves and twice the helpers find work.
        const int parts = shape.coop_parts == 2 ? 2 : 1;
        double share = dc.coop_frac;
        {
            double first = 0.0;
            for (int c = 1; c <= std::min(nc, col_waves); ++c) first += in.col_len[c];
            if (first < 0.5 * dc.coop_frac * terms) {
                max_cols = DEV_MAX_RANGES * col_waves;
                share = 0.92 * dc.coop_frac;  // (several columns per wave: a job is longer for the same share; 35 / 38 / 42 columns at 150x150: 9.24 / 9.04 / 9.72 s)
            }
        }
        if (parts == 2 && max_cols > col_waves) max_cols = 2 * DEV_MAX_RANGES * col_waves;  // (each part has its own DEV_MAX_RANGES per wave)
        if (in.tune.coop_max_columns > 0) max_cols = std::min(parts * DEV_MAX_RANGES * col_waves, (int)in.tune.coop_max_columns);
        // Balanced dealing (round 5; one-part hand-off of a field whose helper jobs hold ONE long column per wave, i.e. 70x70):
        // the column waves of a helper are not alike - the two SIMDs that host the producer and the answering wave run three of them,
        // the other two four - and with the streamed table a helper is bound by its SIMDs' issue, so a wave of a three-wave SIMD walks
        // 4/3 the rows of the others in the same time.  The longest columns still go one per wave; when the share asks for more than
        // those, the FAST waves get a second, medium column each out of one contiguous block of the table (the owners keep contiguous
        // runs on either side), chosen so that every SIMD of the helper finishes together.
        const bool balanced = parts == 1 && max_cols == col_waves && nc > 3 * col_waves;
        std::vector<int> topup;
        if (balanced) {
            double first = 0.0;
            for (int c = 1; c <= col_waves; ++c) first += in.col_len[c];
            const double extra = share * terms - first;
            const int n_fast = 6;
            const double per = extra / n_fast - kCoopStartRows;  // rows of the second column of a fast wave
            if (per >= 6.0) {
                // columns of `per` rows: col_len[c] = deg + 2 - c
                int c_mid = dc.deg + 2 - (int)(per + 0.5);
                int c_lo = c_mid - n_fast / 2, c_hi = c_lo + n_fast - 1;
                if (c_lo <= col_waves) { c_lo = col_waves + 1; c_hi = c_lo + n_fast - 1; }
                if (c_hi > nc - 2) { c_hi = nc - 2; c_lo = c_hi - n_fast + 1; }
                if (c_lo > col_waves)
                    for (int c = c_lo; c <= c_hi; ++c) topup.push_back(c);
            }
        }
        int n_long = 0;  // columns taken from the head of the table (the longest)
        for (int c = 1; c <= nc; ++c) {
            const bool is_top = std::find(topup.begin(), topup.end(), c) != topup.end();
            // (with a second column on the fast waves the long block is the full first round: one column per wave)
            const bool long_ok = n_long < max_cols && c < nc - 1 && (!topup.empty() || given + 0.5 * in.col_len[c] <= share * terms) && (topup.empty() || c <= col_waves);
            if (is_top || long_ok) {
                help.push_back(c);
                given += in.col_len[c];
                if (!is_top) ++n_long;
            } else {
                own.push_back(c);
            }
        }
        // helper: one column per wave, longest first; the two SIMDs that also host the producer and the answering wave have
        // three column waves (4 8 12 / 3 7 11) and take the six longest, the other two SIMDs four each
        static const int wave_order[DEV_MAX_WAVES - 2] = {4, 3, 8, 7, 12, 11, 1, 2, 5, 6, 9, 10, 13, 14};
        for (int part = 0; part < 2; ++part) {
            DevSched &hs = dc.sched[part ? DEV_SCHED_HELPER2 : DEV_SCHED_HELPER];
            for (int w = 0; w < DEV_MAX_WAVES; ++w) hs.n_ranges[w] = 0;
            if (part >= parts) continue;
            std::vector<int> mine;
            for (size_t k = 0; k < help.size(); ++k) if ((int)(k % (size_t)parts) == part) mine.push_back(help[k]);
            if (balanced) {
                // longest column first onto the wave that would finish it soonest: load / speed, speed = kCoopFastWeight on the SIMDs with
                // three column waves (waves 4 8 12 beside the producer, 3 7 11 beside the answering wave)
                double load[DEV_MAX_WAVES] = {0.0};
                for (int c : mine) {  // (ascending column number = descending length)
                    int best = -1;
                    double best_t = 1e300;
                    for (int q = 0; q < col_waves; ++q) {
                        const int w = wave_order[q];
                        if (hs.n_ranges[w] >= DEV_MAX_RANGES) continue;
                        const double speed = (w % 4 == 0 || w % 4 == 3) ? kCoopFastWeight : 1.0;
                        const double t = (load[w] + in.col_len[c] + (hs.n_ranges[w] > 0 ? kCoopStartRows : 0.0)) / speed;
                        if (t < best_t - 1e-9) { best_t = t; best = w; }
                    }
                    if (best < 0) break;
                    load[best] += in.col_len[c] + (hs.n_ranges[best] > 0 ? kCoopStartRows : 0.0);
                    const int r = hs.n_ranges[best]++;
                    hs.range_c0[best][r] = c; hs.range_cnt[best][r] = 1;
                }
                continue;
            }
            for (size_t k = 0; k < mine.size(); ++k) {
                // further rounds are dealt in alternating directions: every wave's set has about the same length
                const int round = (int)k / col_waves, pos = (int)k % col_waves;
                const int w = (round & 1) ? wave_order[col_waves - 1 - pos] : wave_order[pos];
                const int r = hs.n_ranges[w]++;
                hs.range_c0[w][r] = mine[k]; hs.range_cnt[w][r] = 1;
            }
        }
        if (!help.empty() && !own.empty() && fill_schedule(in, dc, quad, dc.sched[DEV_SCHED_PRIMARY], n_waves, own, hc, false)) {
            dc.coop_ok = 1;
        } else {
            dc.coop_ok = 0;
            for (int w = 0; w < DEV_MAX_WAVES; ++w) dc.sched[DEV_SCHED_PRIMARY].n_ranges[w] = dc.sched[DEV_SCHED_HELPER].n_ranges[w] = dc.sched[DEV_SCHED_HELPER2].n_ranges[w] = 0;
        }
    } else {
        dc.coop_ok = 0;
    }
}

// STM layout by ensemble size.  The quad layout spends 4 lanes per trajectory (1.6x the f64 issue slots of the D3 layout
// per trajectory) to get 4x the workgroups and 4x the waves per workgroup: it wins while the D3 layout would leave most of
// the chip without a workgroup, i.e. up to ~2 quad workgroups per CU.
inline bool pick_quad(const PlanInputs &in, const DevCfg &dc, int64_t n) {
    if (!(dc.flags & NYX_HIP_FLAG_STM)) return false;
    if (dc.flags & NYX_HIP_FLAG_STM_TEXTBOOK) return false;  // (the variational equations are integrated by the 64-lane layout: one trajectory's k-buffer column per lane)
    if (in.forced_quad >= 0) return in.forced_quad != 0;
    if (in.tune.stm_quad >= 0) return in.tune.stm_quad != 0;
    // deterministic: the layout fixes the column split, hence the bits - it must not follow the batch size (a shard is a smaller batch)
    if (in.tune.deterministic) return true;
    const int64_t cus = in.n_cu > 0 ? in.n_cu : 256;
    return (n + 15) / 16 <= 2 * cus;
}

// Whether the covariance-mapping loop of n trajectories (nyx_hip_predict_until) runs in ONE launch.  Quad layout only: sixteen waves
// share sixteen trajectories' updates; in the 64-lane layout, the large-ensemble shape, the per-launch cost is a small share and sixteen
// serial updates per wave cost more (26.2 ms fused against 24.3 ms per segment at n = 1 000).  Not with an integration-frame swap
// (translated in and out per segment); debug_flags 0x20000000 keeps the launch per segment as the A/B reference.
inline bool predict_fused(const PlanInputs &in, const DevCfg &dc, int64_t n, int swap_n_chain) {
    return swap_n_chain == 0 && !(in.tune.debug_flags & 0x20000000) && pick_quad(in, dc, n);
}
// Whether the column weights of a workgroup shape (`key`, `n_waves` waves) are measured on the device before n trajectories are
// launched with it.  The two callers differ on purpose.  A launch measures on its own first steps: a plain request only (`plain`: no
// calibration launch itself, no dense output, per-trajectory durations or stop condition), min_n 64, min_steps 100 initial steps.  The
// segment launches of a covariance-mapping loop carry a per-trajectory duration array and are too short to calibrate on themselves:
// their shape is measured once before the loop, whatever the span (min_steps 0), from one quad workgroup on (min_n 16).
inline bool calibrates_first(const PlanInputs &in, const DevCfg &dc, const WKey &key, int n_waves, int64_t n, int64_t min_n, bool plain, int64_t span_ns, int64_t min_steps) {
    return plain && in.tune.schedule == NYX_HIP_SCHED_CALIBRATED && dc.has_grav && n_waves >= 8 && n >= min_n && span_ns >= min_steps * dc.init_step_ns && !in.weights.count(key);
}

inline int pick_waves(const PlanInputs &in, const DevCfg &dc, int64_t n) {
    const bool stm = (dc.flags & NYX_HIP_FLAG_STM) != 0;
    if (stm && pick_quad(in, dc, n)) {  // quad layout: 128 VGPRs per wave like the plain kernel
        if (in.forced_waves > 0) return std::min(in.forced_waves, DEV_MAX_WAVES);
        if (!dc.has_grav) return want_fanout(in, dc, true) ? (fanout_role_waves(dc) > 4 ? 8 : std::max(3, fanout_role_waves(dc))) : 3;
        return dc.deg < 8 ? 8 : 16;
    }
    if (stm) {  // dual-number variant: 256 VGPRs per wave, at most DEV_MAX_WAVES_STM waves
        if (in.forced_waves > 0) return std::min(in.forced_waves, DEV_MAX_WAVES_STM);
        return dc.has_grav ? DEV_MAX_WAVES_STM : 3;
    }
    if (in.forced_waves > 0) return std::min(in.forced_waves, DEV_MAX_WAVES);
    // no harmonics: integrator + almanac + perturbation waves form a 3-stage pipeline
    if (!dc.has_grav) {
        if (!(dc.n_slots > 0 || dc.has_drag || dc.has_tides)) return 1;
        return want_fanout(in, dc, false) ? (fanout_role_waves(dc) > 4 ? 8 : std::max(3, fanout_role_waves(dc))) : 3;  // (8: two role waves per SIMD can be placed)
    }
    // Sixteen waves whatever the ensemble size: a workgroup's LDS (~150 KB) gives it a CU to itself, so the column split is what puts
    // four waves on every SIMD.  (Rounds 1-3 went down to eight and four waves for >= 32 705 / >= 131 009 trajectories, sized when a
    // workgroup was small enough to share a CU; measured in round 4 on configs[1]'s force model, 1 h: 32 768 trajectories 104.2 ms
    // with eight waves against 69.1 with sixteen, 131 072: 521 (four) / 410 (eight) / 277 ms (sixteen) - 0.44 / 0.56 / 0.83 of the
    // FP64 peak.)  The shape therefore depends on the configuration alone, which is also what tuning.deterministic promises.
    (void)n;
    const int deg = dc.deg;
    int want = 16;
    if (deg < 8) want = std::min(want, 4);
    else if (deg < 24) want = std::min(want, 8);
    return want;
}

// Cooperative mode of a launch of n trajectories in nw-wave workgroups: when the trajectory-owning workgroups leave CUs idle, helper
// workgroups take over a share of the harmonics columns (propagate_kernel.hip).  Rebuilds the schedules in `dc` when the mode differs
// from the one `shape` records (and sets `rebuilt`).  Besides (configuration, tuning, n, n_cu) the plan depends on ONE thing a previous
// plan left: dc.coop_frac, the claim mode's helper share, which is re-derived only when it moves by more than 0.01 (hysteresis: a
// share that follows every launch size would rebuild - and re-round - the schedules on every small change of the batch).
inline CoopPlan plan_cooperation(const PlanInputs &in, DevCfg &dc, int64_t n, int nw, SchedShape &shape, bool &rebuilt) {
    CoopPlan cp;
    // on by default; tuning.cooperative = 0 (or .deterministic: the split follows the batch size) makes every workgroup work alone
    const bool want = in.tune.cooperative != 0 && !in.tune.deterministic;
    cp.n_own = (n + DEV_LANES - 1) / DEV_LANES;
    // Helpers start right behind the owners and fill every CU that is left (round 4: 99 helpers instead of 96 for 157 owners is
    // 3.9 % of the north-star run - the helpers' queues are what the owners wait in; rounds 1-3 rounded both to multiples of
    // eight for XCD affinity, which buys nothing measurable).
    cp.base = cp.n_own;
    cp.coop_frac = dc.coop_frac;
    const bool stm = (dc.flags & NYX_HIP_FLAG_STM) != 0;
    if (!(want && !stm && dc.has_grav && dc.g_slot < 0 && nw == DEV_MAX_WAVES && cp.base + 8 <= in.n_cu)) return cp;
    const int64_t n_own = cp.n_own;
    // (more helpers than owners: the jobs are claimed, not assigned, so extra helpers shorten the queue of a set)
    // Two-part hand-off: when the idle CUs outnumber the owners by a quarter and a helper job holds several columns per wave
    // (large fields), every evaluation's hand-off is split in two sub-jobs for two helper workgroups (see build_schedule); the
    // helper count then goes up to two per owner.  (debug_flags 0x80000 forces one part.)
    const int64_t free_cus = in.n_cu - cp.base;
    int claim_parts = (dc.n_cols > 96 && 4 * free_cus >= 5 * n_own) ? 2 : 1;
    if (in.tune.debug_flags & 0x80000) claim_parts = 1;
    double h_ratio = claim_parts == 2 ? 2.0 : 1.0;
    if (in.tune.coop_helper_ratio > 0.0) h_ratio = std::min(3.0, std::max(0.25, in.tune.coop_helper_ratio));
    // Fan-out mode (round 6): when the idle CUs outnumber the owners at least two to one - what a rank runs when ONE ensemble is
    // cut over the GPUs of a node (configs[1] over 2 / 4 / 8 ranks: 79 / 40 / 20 owners), or a small Monte Carlo - every owner gets
    // K = idle CUs / owners (<= DEV_FAN_MAX) DEDICATED helper workgroups and hands them all but its shortest columns.  Measured
    // before it existed (round 6, profiles/round06_shard_sizes_before.log): 5 000 / 2 500 / 1 250 trajectories x 24 h ran
    // 648 / 642 / 639 ms against 615 for 10 000 - a rank of 8 was no faster than one GPU alone.  Fields up to degree 95 (larger
    // ones keep the two-part claim mode, whose jobs hold several columns per wave).  debug_flags 0x8000000 switches it off.
    // It ignores tuning.coop_fraction: the owner keeps only its shortest columns.
    cp.fan = dc.n_cols <= 96 && free_cus >= 2 * n_own && n_own >= 1 && !(in.tune.debug_flags & 0x8000000) &&
             !(in.tune.debug_flags & 0x80000) && !(in.tune.coop_helper_ratio > 0.0);
    cp.parts = cp.fan ? (int)std::min<int64_t>(DEV_FAN_MAX, free_cus / n_own) : claim_parts;
    auto build = [&]() {
        if (cp.parts == shape.coop_parts && cp.fan == shape.coop_fan) return;
        shape.coop_parts = cp.parts;
        shape.coop_fan = cp.fan;
        build_schedule(in, dc, shape, nw);
        rebuilt = true;
    };
    build();
    if (cp.fan && !dc.coop_ok) {  // (a fan-out schedule that does not fit DEV_MAX_RANGES: the claim mode, in this launch)
        cp.fan = false;
        cp.parts = claim_parts;
        build();
    }
    cp.helpers = cp.fan ? n_own * cp.parts : std::min<int64_t>((int64_t)((double)n_own * h_ratio), free_cus);
    if (!cp.fan && !(cp.helpers >= 8 && 4 * cp.helpers >= n_own)) { cp.helpers = 0; return cp; }
    // share of the terms the helpers take: owners keep (1 - x), each helper does x * owners / helpers jobs' worth
    // per evaluation period, plus its hand-off overhead: x ~ 0.95 r / (1 + r) with r = helpers / owners
    if (!cp.fan && !(in.tune.coop_fraction > 0.0)) {
        const double r = (double)cp.helpers / (double)n_own;
        // (two parts, measured on configs[4] with 158 helpers for 98 owners: 0.55 / 0.60 / 0.65 / 0.70 / 0.75 of the terms ->
        //  98.1 / 97.9 / 93.4 / 92.9 / 102.6 ms per hour of the ensemble - half a job per helper takes the knee further out)
        const double x = cp.parts == 2 ? std::min(0.68, std::max(0.10, 1.10 * r / (1.0 + r)))
                                       : std::min(0.55, std::max(0.10, 0.95 * r / (1.0 + r)));
        if (std::fabs(x - dc.coop_frac) > 0.01) {
            dc.coop_frac = x;
            build_schedule(in, dc, shape, nw);
            rebuilt = true;
        }
    }
    cp.coop_frac = dc.coop_frac;
    if (!dc.coop_ok) { cp.helpers = 0; return cp; }
    cp.run = true;
    cp.boxes = n_own;
    cp.answers = cp.fan ? n_own * cp.parts : (cp.parts == 2 ? n_own : 0);
    return cp;
}

// Sixteen-row groups of the run stream of the schedules `ids` (ctx_build.h, build_run_stream, lays out exactly these): every range of
// every wave starts a group of its own, a column's rows go in once, and the walk's look-ahead adds two groups behind the last row.
inline int64_t run_stream_groups(const DevSched *sched, std::initializer_list<int> ids, const std::vector<int32_t> &col_len) {
    int64_t rows = 0;
    std::vector<char> seen(col_len.size(), 0);
    for (int k : ids)
        for (int w = 0; w < DEV_MAX_WAVES; ++w)
            for (int r = 0; r < sched[k].n_ranges[w]; ++r) {
                rows = (rows + 15) / 16 * 16;
                for (int c = sched[k].range_c0[w][r]; c < sched[k].range_c0[w][r] + sched[k].range_cnt[w][r]; ++c) {
                    if (c < 1 || c >= (int)col_len.size() || seen[c]) continue;
                    seen[c] = 1;
                    rows += col_len[c];
                }
            }
    return (rows + 15) / 16 + 2;
}
// The staged block of the helpers' resident feed: {t3..t6} of every group (HYB_GROUP doubles), behind the helper's carve.
inline int64_t helper_stage_bytes(int64_t groups) { return groups * HYB_GROUP * (int64_t)sizeof(double); }
inline bool helper_stage_fits(int64_t groups) { return groups > 0 && helper_stage_bytes(groups) <= DEV_HELPER_STAGE_MAX; }

// The feed of the helpers' column walk in this launch (DevCfg.hres_groups): resident in LDS for the claim-mode helpers of the plain
// sixteen-wave kernel with a one-part hand-off, where the rows of the helper schedule fit (helper_stage_fits) and
// tuning.helper_resident does not say no; the feed of DevCfg.harm_feed everywhere else (two-part hand-offs and the fan-out kernel
// keep theirs).  The same rows through the same operations: the selection moves no bit.  True when dc changed (upload it, and the
// helpers' run stream with it).
inline bool select_helper_feed(const PlanInputs &in, DevCfg &dc, const CoopPlan &cp, int32_t &staged) {
    staged = 0;
    // Only a launch with one-part claim-mode helpers reads dc.hres_groups (its kernel alone carries the resident walk, and the launch's
    // own DevBatch.coop_stage gates it): every other launch leaves the word as it is, so a context that alternates between a
    // cooperative launch and one that works alone rebuilds and uploads nothing for the feed's sake.
    if (!(cp.run && !cp.fan && cp.parts == 1 && dc.n_waves == DEV_MAX_WAVES && !(dc.flags & NYX_HIP_FLAG_STM))) return false;
    int32_t groups = 0;
    if (in.tune.helper_resident != 0) {
        const int64_t g = run_stream_groups(dc.sched, {DEV_SCHED_HELPER, DEV_SCHED_HELPER2}, in.col_len);
        if (helper_stage_fits(g)) groups = (int32_t)g;
    }
    staged = groups;
    if (groups == dc.hres_groups) return false;
    dc.hres_groups = groups;
    return true;
}

// The launch-shape dependent part of a launch of n trajectories: waves per workgroup, STM layout, schedules (rebuilt when the shape
// differs from `shape`, or when `stale`: weights or tuning changed since they were built) and the cooperative mode.
struct LaunchPlan {
    int n_waves = 0;
    bool quad = false;
    bool rebuilt = false;  // the schedules in the DevCfg changed (upload it; rebuild the run streams)
    int32_t staged_groups = 0;  // sixteen-row groups the helpers of THIS launch stage in LDS (select_helper_feed; 0 = none)
    CoopPlan coop;
};
inline LaunchPlan plan_launch(const PlanInputs &in, DevCfg &dc, SchedShape &shape, int64_t n, bool stale) {
    LaunchPlan p;
    p.n_waves = pick_waves(in, dc, n);
    p.quad = pick_quad(in, dc, n);
    if (p.n_waves != dc.n_waves || p.quad != shape.quad || stale) {
        shape.quad = p.quad;
        build_schedule(in, dc, shape, p.n_waves);
        p.rebuilt = true;
    }
    p.coop = plan_cooperation(in, dc, n, p.n_waves, shape, p.rebuilt);
    if (select_helper_feed(in, dc, p.coop, p.staged_groups)) p.rebuilt = true;
    return p;
}

// One fit of calibrate() (abi.cpp): per wave of workgroup 0 of a calibration launch, prof[8 w + 1] = cycles of role work inside the
// window (duty), prof[8 w + 2] = cycles in its columns (harm); c[w] = harm / table entries is what an entry costs THAT wave (the four
// waves of a SIMD are arbitrated oldest first).  The water-filling gets the speed weight cbar / c[w] and the handicap duty[w] / c[w]
// (in entries), which makes duty + columns equal across the waves; damped with `prev`, the previous fit (the shares interact through
// the shared SIMDs); rounded to 1/64.  Not usable when fewer than two waves carried columns or fewer than two had a window.
struct CalibrationFit {
    bool usable = false;
    std::array<double, 2 * DEV_MAX_WAVES> w{};  // speed weights [0..16), duties [16..32) (WeightMap)
    double spread = 0.0;                      // (max - min) / mean of the measured windows
};
inline CalibrationFit calibration_fit(const int64_t *prof, const DevSched &sd, const std::vector<int32_t> &col_len, int nw,
                                      const std::array<double, 2 * DEV_MAX_WAVES> *prev) {
    CalibrationFit f;
    double duty[DEV_MAX_WAVES], harm[DEV_MAX_WAVES], ent[DEV_MAX_WAVES], cpe[DEV_MAX_WAVES];
    double csum = 0.0, lo = 1e300, hi = 0.0, tmean = 0.0;
    int ccnt = 0, tcnt = 0;
    for (int q = 0; q < nw; ++q) {
        duty[q] = (double)prof[q * 8 + 1];
        harm[q] = (double)prof[q * 8 + 2];
        ent[q] = 0.0;
        for (int r = 0; r < sd.n_ranges[q]; ++r)
            for (int c = sd.range_c0[q][r]; c < sd.range_c0[q][r] + sd.range_cnt[q][r]; ++c) ent[q] += col_len[c];
        cpe[q] = (ent[q] > 0.0 && harm[q] > 0.0) ? harm[q] / ent[q] : 0.0;   // cycles per table entry, as this wave sees them
        if (cpe[q] > 0.0) { csum += cpe[q]; ++ccnt; }
        if (q > 0 || nw < 8) {
            const double t = duty[q] + (ent[q] > 0.0 ? harm[q] : 0.0);
            if (t > 0.0) { lo = std::min(lo, t); hi = std::max(hi, t); tmean += t; ++tcnt; }
        }
    }
    if (ccnt < 2 || tcnt < 2) return f;
    const double cbar = csum / ccnt;
    f.spread = (hi - lo) / (tmean / tcnt);
    std::array<double, 2 * DEV_MAX_WAVES> nwgt;
    for (int q = 0; q < DEV_MAX_WAVES; ++q) {
        // a wave that carried no columns this time is given the speed of its SIMD age class (waves q, q+4, q+8, q+12 share a SIMD)
        double c = q < nw ? cpe[q] : 0.0;
        if (!(c > 0.0)) {
            double a = 0.0; int an = 0;
            for (int k = (q / 4) * 4; k < (q / 4) * 4 + 4 && k < nw; ++k) if (cpe[k] > 0.0) { a += cpe[k]; ++an; }
            c = an ? a / an : cbar;
        }
        nwgt[q] = cbar / c;
        nwgt[DEV_MAX_WAVES + q] = q < nw ? duty[q] / c : 0.0;
    }
    for (int q = 0; q < 2 * DEV_MAX_WAVES; ++q) {
        const double v = prev ? 0.5 * ((*prev)[q] + nwgt[q]) : nwgt[q];
        f.w[q] = std::round(v * 64.0) / 64.0;
    }
    f.usable = true;
    return f;
}
