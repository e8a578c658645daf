// Stand-alone check of the batch binding (nyx_amd/csrc/batch_bind.h) and the calibration fit (calibration_fit, launch_plan.h) - g++ only,
// no HIP, no GPU (tests/test_batch_bind.py).
//   batch_bind_check FITS_OUT
// checks the state-row table, bind_batch, slices, shards, the trajectory scatter and the trajectory-block layout, and the weight key of
// the covariance-mapping loop; replays calibrations on synthetic cycle tables over the BASELINE shapes and writes one line per
// calibration to FITS_OUT (compared with tests/golden/calibration_fit.txt by the test: the weights as hex floats).  "ok" last.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../nyx_amd/csrc/batch_bind.h"
#include "../../nyx_amd/csrc/ctx_build.h"
#include "launch_plan_cases.h"

static int g_fail = 0;
#define CHECK(cond, ...)                                                              \
    do {                                                                              \
        if (!(cond)) {                                                                \
            if (++g_fail <= 30) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                             \
    } while (0)

template <typename T> static T *fake(uintptr_t a) { return (T *)a; }

// A nyx_hip_states_t with a distinct fake address in every array: 0x10000 * (base + field number).
static nyx_hip_states_t fake_states(uintptr_t base, int64_t n, bool stm) {
    nyx_hip_states_t s;
    std::memset(&s, 0, sizeof s);
    s.n = n;
    s.epoch_ns = fake<int64_t>(0x10000 * (base + 1));
    s.x_km = fake<double>(0x10000 * (base + 2)); s.y_km = fake<double>(0x10000 * (base + 3)); s.z_km = fake<double>(0x10000 * (base + 4));
    s.vx_km_s = fake<double>(0x10000 * (base + 5)); s.vy_km_s = fake<double>(0x10000 * (base + 6)); s.vz_km_s = fake<double>(0x10000 * (base + 7));
    s.cr = fake<double>(0x10000 * (base + 8)); s.cd = fake<double>(0x10000 * (base + 9)); s.prop_mass_kg = fake<double>(0x10000 * (base + 10));
    s.dry_mass_kg = fake<double>(0x10000 * (base + 11)); s.extra_mass_kg = fake<double>(0x10000 * (base + 12));
    s.srp_area_m2 = fake<double>(0x10000 * (base + 13)); s.drag_area_m2 = fake<double>(0x10000 * (base + 14));
    s.stm = stm ? fake<double>(0x10000 * (base + 15)) : nullptr;
    s.step_ns = fake<int64_t>(0x10000 * (base + 16));
    return s;
}
static nyx_hip_step_stats_t fake_stats(uintptr_t base) {
    return nyx_hip_step_stats_t{fake<int32_t>(0x10000 * (base + 1)), fake<int64_t>(0x10000 * (base + 2)), fake<double>(0x10000 * (base + 3)),
                                fake<int32_t>(0x10000 * (base + 4)), fake<int64_t>(0x10000 * (base + 5)), fake<int64_t>(0x10000 * (base + 6)),
                                fake<int64_t>(0x10000 * (base + 7))};
}
static nyx_hip_traj_t fake_traj(uintptr_t base, int64_t cap) {
    return nyx_hip_traj_t{cap, fake<int64_t>(0x10000 * (base + 1)), fake<double>(0x10000 * (base + 2)), fake<double>(0x10000 * (base + 3)),
                          fake<double>(0x10000 * (base + 4)), fake<double>(0x10000 * (base + 5)), fake<double>(0x10000 * (base + 6)),
                          fake<double>(0x10000 * (base + 7)), fake<int32_t>(0x10000 * (base + 8))};
}

// ---- the row table: every double * member of nyx_hip_states_t once, in header order, and the DevBatch rows that receive them
static void check_rows() {
    const nyx_hip_states_t s = fake_states(100, 7, true);
    const double *const members[13] = {s.x_km, s.y_km, s.z_km, s.vx_km_s, s.vy_km_s, s.vz_km_s, s.cr, s.cd, s.prop_mass_kg, s.dry_mass_kg,
                                       s.extra_mass_kg, s.srp_area_m2, s.drag_area_m2};
    CHECK(kStateRows == 13 && kCartRows == 6 && kMomentRows == 9, "row counts");
    // the double * members of the struct, by offset: x_km .. drag_area_m2 are contiguous and the table walks them in order
    const size_t first = offsetof(nyx_hip_states_t, x_km), last = offsetof(nyx_hip_states_t, drag_area_m2);
    CHECK((last - first) / sizeof(double *) + 1 == 13, "13 rows between x_km and drag_area_m2");
    for (int k = 0; k < kStateRows; ++k) {
        CHECK(s.*kStateRow[k].s == members[k], "row %d", k);
        nyx_hip_states_t probe;
        CHECK((const char *)&(probe.*kStateRow[k].s) - (const char *)&probe == (ptrdiff_t)(first + k * sizeof(double *)), "row %d: header order", k);
    }
    DevBatch bt;
    std::memset(&bt, 0, sizeof bt);
    for (int k = 0; k < kStateRows; ++k) { bt.*kStateRow[k].in = members[k]; bt.*kStateRow[k].out = (double *)members[k] + 1; }
    const double *in[13] = {bt.x, bt.y, bt.z, bt.vx, bt.vy, bt.vz, bt.cr, bt.cd, bt.mprop, bt.mdry, bt.mextra, bt.asrp, bt.adrag};
    const double *out[13] = {bt.o_x, bt.o_y, bt.o_z, bt.o_vx, bt.o_vy, bt.o_vz, bt.o_cr, bt.o_cd, bt.o_mprop, bt.o_mdry, bt.o_mextra, bt.o_asrp, bt.o_adrag};
    for (int k = 0; k < kStateRows; ++k) CHECK(in[k] == members[k] && out[k] == members[k] + 1, "DevBatch row %d", k);
    const nyx_hip_traj_t t = fake_traj(300, 4);
    const double *trows[6] = {t.x_km, t.y_km, t.z_km, t.vx_km_s, t.vy_km_s, t.vz_km_s};
    for (int c = 0; c < kCartRows; ++c) CHECK(t.*kTrajRow[c] == trows[c], "traj row %d", c);
}

// ---- bind_batch: every DevBatch field against a table written out here
static DevBatch expected_plain(const nyx_hip_states_t &i, const nyx_hip_states_t &o, const nyx_hip_step_stats_t &st) {
    DevBatch e;
    std::memset(&e, 0, sizeof e);
    e.n = i.n; e.duration_ns = 3600000000000LL;
    e.epoch_ns = i.epoch_ns;
    e.x = i.x_km; e.y = i.y_km; e.z = i.z_km; e.vx = i.vx_km_s; e.vy = i.vy_km_s; e.vz = i.vz_km_s; e.cr = i.cr; e.cd = i.cd;
    e.mprop = i.prop_mass_kg; e.mdry = i.dry_mass_kg; e.mextra = i.extra_mass_kg; e.asrp = i.srp_area_m2; e.adrag = i.drag_area_m2;
    e.step_in = i.step_ns;
    e.o_epoch_ns = o.epoch_ns;
    e.o_x = o.x_km; e.o_y = o.y_km; e.o_z = o.z_km; e.o_vx = o.vx_km_s; e.o_vy = o.vy_km_s; e.o_vz = o.vz_km_s; e.o_cr = o.cr; e.o_cd = o.cd;
    e.o_mprop = o.prop_mass_kg; e.o_mdry = o.dry_mass_kg; e.o_mextra = o.extra_mass_kg; e.o_asrp = o.srp_area_m2; e.o_adrag = o.drag_area_m2;
    e.o_step = o.step_ns;
    e.status = st.status; e.last_step_ns = st.last_step_ns; e.last_error = st.last_error; e.last_attempts = st.last_attempts;
    e.n_acc = st.n_accepted; e.n_rej = st.n_rejected; e.n_evals = st.n_evals;
    return e;
}
static void same_batch(const BoundBatch &b, const DevBatch &e, const char *tag) {
    CHECK(b.rc == NYX_HIP_RC_OK && b.error == nullptr, "%s: refused", tag);
    CHECK(std::memcmp(&b.bt, &e, sizeof e) == 0, "%s: bound DevBatch differs", tag);
}
static void check_bind() {
    nyx_hip_states_t i = fake_states(1000, 640, true), o = fake_states(2000, 640, true);
    nyx_hip_step_stats_t st = fake_stats(3000);
    LaunchReq r;
    r.in = &i; r.out = &o; r.stats = &st; r.duration_ns = 3600000000000LL;
    {   // plain: no STMs even though the states carry them, no stats pointers when there are no stats
        DevBatch e = expected_plain(i, o, st);
        same_batch(bind_batch(r, false, nullptr), e, "plain");
        LaunchReq r2 = r;
        r2.stats = nullptr;
        e.status = nullptr; e.last_step_ns = nullptr; e.last_error = nullptr; e.last_attempts = nullptr; e.n_acc = nullptr; e.n_rej = nullptr; e.n_evals = nullptr;
        same_batch(bind_batch(r2, false, nullptr), e, "plain, no stats");
    }
    {
        DevBatch e = expected_plain(i, o, st);
        e.stm = i.stm; e.o_stm = o.stm;
        same_batch(bind_batch(r, true, nullptr), e, "stm");
    }
    {
        const nyx_hip_traj_t t = fake_traj(4000, 12);
        LaunchReq r2 = r;
        r2.traj = &t;
        DevBatch e = expected_plain(i, o, st);
        e.traj_cap = 12; e.t_epoch = t.epoch_ns; e.t_len = t.len;
        e.t_state[0] = t.x_km; e.t_state[1] = t.y_km; e.t_state[2] = t.z_km; e.t_state[3] = t.vx_km_s; e.t_state[4] = t.vy_km_s; e.t_state[5] = t.vz_km_s;
        same_batch(bind_batch(r2, false, nullptr), e, "dense output");
        const nyx_hip_traj_t t0 = fake_traj(4000, 0);  // capacity 0: no dense output
        r2.traj = &t0;
        same_batch(bind_batch(r2, false, nullptr), expected_plain(i, o, st), "dense output, capacity 0");
    }
    {
        DevBatch ev;
        std::memset(&ev, 0, sizeof ev);
        ev.ev = fake<nyx_hip_event_t>(0x50000); ev.ev_mu = 398600.4415; ev.ev_prev = fake<double>(0x51000);
        ev.ev_count = fake<int32_t>(0x52000); ev.ev_found = fake<int32_t>(0x53000);
        ev.n = 99; ev.x = fake<double>(0x54000);  // (not read: only the ev_* fields of a stop condition are)
        LaunchReq r2 = r;
        r2.ev = &ev;
        DevBatch e = expected_plain(i, o, st);
        e.ev_on = 1; e.ev = ev.ev; e.ev_mu = 398600.4415; e.ev_prev = ev.ev_prev; e.ev_count = ev.ev_count; e.ev_found = ev.ev_found;
        same_batch(bind_batch(r2, false, nullptr), e, "stop condition");
    }
    {
        const int64_t *dur = fake<int64_t>(0x60000);
        const PredictArgs *pred = fake<PredictArgs>(0x61000);
        LaunchReq r2 = r;
        r2.dur_ns = dur; r2.duration_ns = 0;
        DevBatch e = expected_plain(i, o, st);
        e.duration_ns = 0; e.dur_ns = dur; e.pred = pred; e.stm = i.stm; e.o_stm = o.stm;
        same_batch(bind_batch(r2, true, pred), e, "dur_ns");
    }
    {
        LaunchReq r2 = r;
        r2.duration_ns = 0; r2.end_epoch_ns = 851472000000000000LL; r2.use_end = true;
        DevBatch e = expected_plain(i, o, st);
        e.duration_ns = 0; e.end_epoch_ns = 851472000000000000LL; e.use_end_epoch = 1;
        same_batch(bind_batch(r2, false, nullptr), e, "end epoch");
    }
    for (int which = 0; which < 2; ++which) {  // the STM refusal: either array missing
        nyx_hip_states_t i2 = i, o2 = o;
        (which ? o2 : i2).stm = nullptr;
        LaunchReq r2 = r;
        r2.in = &i2; r2.out = &o2;
        const BoundBatch b = bind_batch(r2, true, nullptr);
        CHECK(b.rc == NYX_HIP_RC_BAD_ARG && b.error && std::string(b.error) == "STM context: in->stm and out->stm are mandatory", "stm refusal %d", which);
        CHECK(bind_batch(r2, false, nullptr).rc == NYX_HIP_RC_OK, "no STM context: the STMs are not read %d", which);
    }
    for (int which = 0; which < 8; ++which) {  // the dense-output refusal: any of its eight arrays missing
        nyx_hip_traj_t t = fake_traj(4000, 12);
        int64_t **ep = &t.epoch_ns;
        int32_t **len = &t.len;
        if (which == 0) *ep = nullptr; else if (which == 7) *len = nullptr; else t.*kTrajRow[which - 1] = nullptr;
        LaunchReq r2 = r;
        r2.traj = &t;
        const BoundBatch b = bind_batch(r2, false, nullptr);
        CHECK(b.rc == NYX_HIP_RC_BAD_ARG && b.error && std::string(b.error) == "traj: every array is mandatory", "traj refusal %d", which);
    }
}

// ---- slices, shards, the scatter, the trajectory block
static void check_slices() {
    nyx_hip_states_t s = fake_states(500, 1000, true);
    s.cd = nullptr; s.step_ns = nullptr;
    const nyx_hip_states_t v = states_at(s, 37, 100);
    CHECK(v.n == 100 && v.epoch_ns == s.epoch_ns + 37 && v.stm == s.stm + 37 * 81 && v.step_ns == nullptr, "states_at");
    for (int k = 0; k < kStateRows; ++k) CHECK(v.*kStateRow[k].s == (s.*kStateRow[k].s ? s.*kStateRow[k].s + 37 : nullptr), "states_at row %d", k);
    s.stm = nullptr;
    CHECK(states_at(s, 37, 100).stm == nullptr, "states_at: no STM");
    nyx_hip_step_stats_t st = fake_stats(600);
    st.last_error = nullptr;
    const nyx_hip_step_stats_t w = stats_at(st, 11);
    CHECK(w.status == st.status + 11 && w.last_step_ns == st.last_step_ns + 11 && w.last_error == nullptr && w.last_attempts == st.last_attempts + 11 &&
          w.n_accepted == st.n_accepted + 11 && w.n_rejected == st.n_rejected + 11 && w.n_evals == st.n_evals + 11, "stats_at");
    for (int64_t n : {0, 1, 7, 10000})
        for (int64_t m = 1; m <= 8; ++m) {
            int64_t covered = 0;
            for (int64_t k = 0; k < m; ++k) {
                const int64_t lo = shard_begin(n, k, m), hi = shard_begin(n, k + 1, m);
                CHECK(lo == n * k / m && lo == covered && hi >= lo, "shard %lld of %lld, n = %lld", (long long)k, (long long)m, (long long)n);
                covered = hi;
            }
            CHECK(covered == n && shard_begin(n, 0, m) == 0, "shards of %lld over %lld", (long long)n, (long long)m);
        }
    CHECK(shard_begin(10, 1, 4) - shard_begin(10, 0, 4) == 2 && shard_begin(10, 2, 4) - shard_begin(10, 1, 4) == 3, "n = 10, m = 4: 2/3/2/3");
    for (int64_t cap : {1, 3})  // the scatter against a naive loop
        for (int64_t n : {1, 7, 50}) {
            std::vector<int64_t> ep((size_t)(cap * n), -1);
            std::vector<double> rows[6];
            std::vector<int32_t> len((size_t)n, -1);
            for (auto &r : rows) r.assign((size_t)(cap * n), -1.0);
            nyx_hip_traj_t batch{cap, ep.data(), rows[0].data(), rows[1].data(), rows[2].data(), rows[3].data(), rows[4].data(), rows[5].data(), len.data()};
            for (int64_t m_ctx = 1; m_ctx <= 3; ++m_ctx)
                for (int64_t k = 0; k < m_ctx; ++k) {
                    const int64_t lo = shard_begin(n, k, m_ctx), m = shard_begin(n, k + 1, m_ctx) - lo;
                    if (!m) continue;
                    std::vector<double> blk((traj_block_bytes(cap, m) + 7) / 8);
                    const nyx_hip_traj_t sh = traj_in_block(blk.data(), cap, m);
                    for (int64_t q = 0; q < cap * m; ++q) {
                        sh.epoch_ns[q] = 1000 * m_ctx + q;
                        for (int c = 0; c < 6; ++c) (sh.*kTrajRow[c])[q] = 100.0 * c + 0.5 * q + m_ctx;
                    }
                    for (int64_t q = 0; q < m; ++q) sh.len[q] = (int32_t)(7 * q + m_ctx);
                    scatter_traj(sh, lo, m, batch, n);
                    bool ok = true;
                    for (int64_t i = 0; i < m; ++i) {
                        ok = ok && len[(size_t)(lo + i)] == sh.len[i];
                        for (int64_t s2 = 0; s2 < cap; ++s2) {
                            ok = ok && ep[(size_t)(s2 * n + lo + i)] == sh.epoch_ns[s2 * m + i];
                            for (int c = 0; c < 6; ++c) ok = ok && rows[c][(size_t)(s2 * n + lo + i)] == (sh.*kTrajRow[c])[s2 * m + i];
                        }
                    }
                    CHECK(ok, "scatter cap %lld n %lld shard %lld/%lld", (long long)cap, (long long)n, (long long)k, (long long)m_ctx);
                }
        }
    for (int64_t cap : {0, 1, 2, 9})  // the block against both layouts of the parent: DevTraj::alloc and host_propagate's
        for (int64_t n : {1, 3, 640}) {
            char *base = fake<char>(0x100000);
            const nyx_hip_traj_t t = traj_in_block(base, cap, n);
            const size_t slots = (size_t)cap * (size_t)n, s1 = std::max<size_t>(slots, 1);
            double *b1 = (double *)base + s1;  // DevTraj::alloc
            CHECK(traj_block_bytes(cap, n) == s1 * 7 * sizeof(double) + (size_t)n * sizeof(int32_t) && t.capacity == cap && t.epoch_ns == (int64_t *)base &&
                  t.x_km == b1 && t.y_km == b1 + slots && t.z_km == b1 + 2 * slots && t.vx_km_s == b1 + 3 * slots && t.vy_km_s == b1 + 4 * slots &&
                  t.vz_km_s == b1 + 5 * slots && t.len == (int32_t *)(b1 + 6 * s1), "DevTraj layout cap %lld n %lld", (long long)cap, (long long)n);
            if (cap < 1) continue;
            double *b2 = (double *)base + slots;  // host_propagate
            CHECK(traj_block_bytes(cap, n) == slots * 7 * sizeof(double) + (size_t)n * sizeof(int32_t) && t.x_km == b2 && t.y_km == b2 + slots &&
                  t.z_km == b2 + 2 * slots && t.vx_km_s == b2 + 3 * slots && t.vy_km_s == b2 + 4 * slots && t.vz_km_s == b2 + 5 * slots &&
                  t.len == (int32_t *)(b2 + 6 * slots), "host_propagate layout cap %lld n %lld", (long long)cap, (long long)n);
        }
}

// ---- a context as far as the planner goes (tests/cxx/launch_plan_check.cpp)
struct Ctx {
    nyx_hip_tuning_t tune;
    std::unique_ptr<DevCfg> dc{new DevCfg};
    std::vector<int32_t> col_len;
    double rh[3] = {0.0, 0.0, 0.0};
    int terms2 = 0, ed_reuse_fit = 0, n_cu = 256;
    WeightMap weights;
    SchedShape shape;
    PlanInputs in() const { return PlanInputs{tune, col_len, rh, terms2, ed_reuse_fit, n_cu, 0, -1, weights}; }
};
static bool create(Ctx &c, const nyx_hip_config_t &cfg, const nyx_hip_tuning_t &tune) {
    c.tune = tune;
    CtxBuild b;
    if (build_context(cfg, tune, lpc::lds_room, b) != NYX_HIP_RC_OK) { std::printf("FAIL build: %s\n", b.error.c_str()); ++g_fail; return false; }
    std::memcpy(c.dc.get(), &b.dc, sizeof(DevCfg));
    c.col_len = b.col_len; c.terms2 = b.terms2; c.ed_reuse_fit = b.ed_reuse_fit;
    std::memcpy(c.rh, b.role_handicap, sizeof c.rh);
    plan_first_schedule(c.in(), *c.dc, c.shape, b.harm_feed);
    return true;
}

// ---- the calibration fit: calibrations replayed launch by launch as calibrate() (abi.cpp) runs them, each launch planned as launch()
// plans it, its cycle table synthetic
// Synthetic cycle tables of a calibration launch: prof[8 w + 1] = duty, prof[8 w + 2] = harm of wave w of workgroup 0 (the rest of
// the 17 x 8 table zero).  kind 'A': every wave busy; 'Z': every third wave measured no harmonics cycles (age-class fill); 'S': windows
// within ~1 % (the spread stop); 'C': one wave with columns measured cycles (fewer than two waves to fit); 'T': only the first two waves
// with columns measured, no duties (fewer than two windows when one of them is wave 0 of a wide workgroup).
inline std::vector<int64_t> synth_table(char kind, uint32_t seed, int nw, const DevSched &sd, const std::vector<int32_t> &col_len) {
    std::vector<int64_t> prof(17 * 8, 0);
    uint32_t x = seed * 2654435761u + 12345u;
    auto rnd = [&](int m) { x = x * 1664525u + 1013904223u; return (int64_t)((x >> 8) % (uint32_t)m); };
    int with_cols = 0;
    for (int q = 0; q < nw; ++q) {
        int64_t ent = 0;
        for (int r = 0; r < sd.n_ranges[q]; ++r)
            for (int c = sd.range_c0[q][r]; c < sd.range_c0[q][r] + sd.range_cnt[q][r]; ++c) ent += col_len[c];
        int64_t duty = (q < 3 ? 3000 + 1500 * q : 0) + rnd(700), harm = ent > 0 ? 40 * ent + 9000 + 400 * (q % 4) + rnd(3000) : rnd(50);
        if (kind == 'Z' && q % 3 == 2) harm = 0;
        if (kind == 'S') harm = std::max<int64_t>(0, 60000 - duty + rnd(500));
        if (kind == 'C') harm = (ent > 0 && with_cols == 0) ? harm : 0;
        if (kind == 'T') { duty = 0; harm = (ent > 0 && with_cols < 2) ? harm : 0; }
        with_cols += ent > 0;
        prof[(size_t)q * 8] = 1000000 + rnd(1000);  // (column 0: the window, not read by the fit)
        prof[(size_t)q * 8 + 1] = duty;
        prof[(size_t)q * 8 + 2] = harm;
    }
    return prof;
}
struct CalCase { const char *shape; int64_t n; const char *tables; };
// Calibrations replayed: the shape (tests/cxx/launch_plan_cases.h), the ensemble size and the table of every launch in turn (then 'C':
// unusable, which ends a calibration that is still going).
static const CalCase kCalCases[] = {
    {"cfg2_70x70", 640, "A"}, {"cfg2_70x70", 640, "Z"}, {"cfg2_70x70", 640, "AS"}, {"cfg2_70x70", 640, "AZ"}, {"cfg2_70x70", 640, "AZS"},
    {"cfg2_70x70", 640, "C"}, {"cfg2_70x70", 640, "T"}, {"cfg2_70x70", 16384, "A"}, {"cfg2_70x70", 16384, "Z"}, {"cfg2_70x70", 16384, "AS"},
    {"cfg2_70x70", 16384, "AZ"}, {"cfg2_70x70", 16384, "C"}, {"cfg2_70x70", 16384, "T"}, {"cfg5_150x150", 640, "A"}, {"cfg5_150x150", 640, "AS"},
    {"cfg5_150x150", 16384, "A"}, {"cfg5_150x150", 16384, "ZA"}, {"deg21", 16384, "A"}, {"deg21", 16384, "Z"}, {"deg21", 16384, "AS"},
    {"deg21", 16384, "AZ"}, {"deg21", 16384, "C"}, {"deg21", 16384, "T"}, {"deg21", 640, "A"}, {"deg21", 640, "ZS"},
    {"cfg4_stm21", 640, "A"}, {"cfg4_stm21", 640, "AS"}, {"cfg4_stm21", 640, "Z"}, {"cfg4_stm21", 640, "T"}, {"cfg4_stm21", 16384, "A"},
    {"cfg4_stm21", 16384, "Z"}, {"cfg4_stm21", 16384, "AS"}, {"cfg4_stm21", 16384, "AZ"}, {"cfg4_stm21", 16384, "C"}, {"cfg4_stm21", 16384, "T"},
    {"cfg3_jwst", 640, "A"}, {"grav2_70+10", 16384, "A"}, {"grav2_70+10", 640, "AZ"},
};
static void write_fits(FILE *f) {
    const std::vector<lpc::Shape> shapes = lpc::shapes();
    for (const CalCase &cc : kCalCases) {
        const lpc::Shape *sh = nullptr;
        for (const lpc::Shape &s : shapes) if (s.name == cc.shape) sh = &s;
        Ctx c;
        if (!sh || !create(c, sh->cfg->cfg, NYX_HIP_TUNING_DEFAULT)) { std::printf("FAIL %s\n", cc.shape); ++g_fail; continue; }
        const std::string tables = cc.tables;
        CalibrationFit fit;
        WKey key(0, 0, 0, 0);
        int nw = 0;
        for (int it = 0; it < 4; ++it) {
            if (fit.usable) c.weights[key] = fit.w;
            const LaunchPlan p = plan_launch(c.in(), *c.dc, c.shape, cc.n, fit.usable);
            key = weight_key(*c.dc, p.n_waves, p.quad, p.coop.run);
            nw = p.n_waves;
            const DevSched &sd = c.dc->sched[std::get<3>(key) >= 0 ? DEV_SCHED_PRIMARY : DEV_SCHED_SOLO];
            const char kind = it < (int)tables.size() ? tables[(size_t)it] : 'C';
            const std::vector<int64_t> prof = synth_table(kind, (uint32_t)(it * 7 + tables.size() * 131 + cc.n), nw, sd, c.col_len);
            const CalibrationFit g = calibration_fit(prof.data(), sd, c.col_len, nw, fit.usable ? &fit.w : nullptr);
            if (!g.usable) break;
            fit = g;
            if (it > 0 && fit.spread < 0.08) break;
        }
        std::fprintf(f, "%s n=%lld %s nw=%d", cc.shape, (long long)cc.n, cc.tables, nw);
        if (!fit.usable) { std::fprintf(f, " usable=0\n"); continue; }
        std::fprintf(f, " usable=1 spread=%a w=", fit.spread);
        for (double v : fit.w) std::fprintf(f, "%a,", v);
        std::fprintf(f, "\n");
    }
}

// ---- the weight key of the covariance-mapping loop: planned (launch()'s key) against the hand-written key it replaces
static void check_predict_key() {
    struct V { const char *name; bool corner; std::unique_ptr<lpc::Config> cfg; nyx_hip_tuning_t tune; };
    std::vector<V> vs;
    vs.push_back(V{"cfg4_stm21", false, lpc::earth_sun_moon(21, NYX_HIP_FLAG_STM), NYX_HIP_TUNING_DEFAULT});
    vs.push_back(V{"stm70", false, lpc::earth_sun_moon(70, NYX_HIP_FLAG_STM), NYX_HIP_TUNING_DEFAULT});
    vs.push_back(V{"cfg4_stm21+merge_roles", true, lpc::earth_sun_moon(21, NYX_HIP_FLAG_STM), NYX_HIP_TUNING_DEFAULT});
    vs.back().tune.merge_roles = 1;
    vs.push_back(V{"stm21, field of the Moon", true, lpc::earth_sun_moon(21, NYX_HIP_FLAG_STM), NYX_HIP_TUNING_DEFAULT});
    lpc::set_field(*vs.back().cfg, 0, 21, lpc::MOON + 1);
    int corner_differs = 0;
    for (V &v : vs)
        for (int64_t n : lpc::kSizes) {
            Ctx c;
            if (!create(c, v.cfg->cfg, v.tune)) continue;
            const int nw_c = pick_waves(c.in(), *c.dc, n);  // the parent's key
            const bool quad_c = pick_quad(c.in(), *c.dc, n);
            const bool pipe_c = quad_c && nw_c == DEV_MAX_WAVES && v.tune.pipelined != 0;
            const WKey old_key(nw_c, pipe_c ? 1 : 0, quad_c ? 1 : 0, -1);
            const std::unique_ptr<DevCfg> dc(new DevCfg(*c.dc));
            SchedShape shape = c.shape;
            const LaunchPlan p = plan_launch(c.in(), *dc, shape, n, true);
            const WKey key = weight_key(*dc, p.n_waves, p.quad, p.coop.run);
            const bool differs = key != old_key;
            CHECK(differs == (v.corner && pipe_c), "%s n=%lld: keys (%d,%d,%d,%d) / (%d,%d,%d,%d)", v.name, (long long)n, std::get<0>(key), std::get<1>(key),
                  std::get<2>(key), std::get<3>(key), std::get<0>(old_key), std::get<1>(old_key), std::get<2>(old_key), std::get<3>(old_key));
            if (differs) CHECK(std::get<1>(key) == 0 && std::get<1>(old_key) == 1, "%s: only the pipe bit", v.name);
            corner_differs += differs;
        }
    CHECK(corner_differs > 0, "the corner cases reach the sixteen-wave quad shape");
    std::printf("predict key: %d corner-case shapes differ\n", corner_differs);
}

int main(int argc, char **argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: batch_bind_check FITS_OUT\n"); return 2; }
    check_rows();
    check_bind();
    check_slices();
    check_predict_key();
    FILE *f = std::fopen(argv[1], "w");
    if (!f) return 2;
    write_fits(f);
    std::fclose(f);
    if (g_fail) { std::printf("%d failures\n", g_fail); return 1; }
    std::printf("ok\n");
    return 0;
}
