// abi.cpp — host side of the C-ABI (include/nyx_hip.h): context creation (what it builds: ctx_build.h; the launch policy:
// launch_plan.h; a batch's arrays in a launch: batch_bind.h; refusals and device blocks: run_host.h, series_host.h, stats_host.h,
// lambert_args.h, target_args.h on dev_block.h; the context's memory: ctx_mem.h; here the device, the uploads), batch staging, the two
// host brackets (host_run for the runs, host_block for the flavours whose device arrays are one block) and kernel launch.
// Compiled with hipcc.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <array>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <tuple>
#include <vector>

#include "../../include/nyx_hip.h"
#include "batch_bind.h"
#include "ctx_build.h"
#include "ctx_mem.h"
#include "devcfg.h"
#include "launch_plan.h"
#include "predict_args.h"
#include "traj_args.h"
#include "moments_args.h"
#include "report_args.h"
#include "ric_args.h"
#include "aer_args.h"
#include "eclipse_args.h"
#include "link_args.h"
#include "frame_args.h"
#include "lambert_args.h"
#include "target_args.h"
#include "groundtrack_args.h"
#include "series_host.h"
#include "stats_host.h"
#include "run_host.h"

extern "C" size_t nyx_kernel_lds_bytes(int n_waves, int rec_doubles, int stm, int reuse_fields);
extern "C" hipError_t nyx_launch_predict_init(const PredictArgs *a, const int64_t *epoch0, hipStream_t stream);
extern "C" hipError_t nyx_launch_time_update(const PredictArgs *a, hipStream_t stream);
extern "C" hipError_t nyx_launch_event_search(const EventSearchArgs *args, hipStream_t stream);
extern "C" hipError_t nyx_launch_traj_eval(const TrajEvalArgs *args, hipStream_t stream);
extern "C" hipError_t nyx_launch_traj_values(const ValuesArgs *args, hipStream_t stream);
extern "C" hipError_t nyx_launch_ric_diff(const RicArgs *args, hipStream_t stream);
extern "C" hipError_t nyx_launch_ground_track(const GroundTrackArgs *args, hipStream_t stream);
extern "C" hipError_t nyx_launch_traj_aer(const AerArgs *args, hipStream_t stream);
extern "C" hipError_t nyx_launch_traj_eclipse(const EclArgs *args, const DevSeg *ctx_seg, hipStream_t stream);
extern "C" hipError_t nyx_launch_traj_frame_values(const FrmArgs *args, const DevSeg *ctx_seg, hipStream_t stream);
extern "C" hipError_t nyx_launch_lambert_batch(const LmbBatchArgs *args, hipStream_t stream);
extern "C" hipError_t nyx_launch_lambert_grid(const LmbGridArgs *args, const DevSeg *ctx_seg, hipStream_t stream);
extern "C" hipError_t nyx_launch_target_seed(const TgtArgs *args, hipStream_t stream);
extern "C" hipError_t nyx_launch_target_step(const TgtArgs *args, hipStream_t stream);
extern "C" hipError_t nyx_launch_traj_link(const LnkArgs *args, const DevSeg *ctx_seg, hipStream_t stream);
extern "C" hipError_t nyx_launch_series_stats(const StatArgs *args, int64_t n_rows, hipStream_t stream);
extern "C" hipError_t nyx_launch_moments(const MomArgs &a, double *out, hipStream_t stream);
extern "C" hipError_t nyx_launch_frame_shift(const DevCfg *cfg, const double *records, const int32_t *chain_seg, const double *chain_sign,
                                             int n_chain, int64_t n, const int64_t *epoch_ns, double *x, double *y, double *z, double *vx,
                                             double *vy, double *vz, double dir, int32_t *status, const int32_t *prior, const int64_t *dur_ns,
                                             hipStream_t stream);
extern "C" hipError_t nyx_launch_propagate(const DevBatch &bt, const DevCfg *cfg, const HarmEntry *htab,
                                           const ColHdr *cols, const double *records, int n_waves, int rec_lds_doubles,
                                           int reuse_fields, hipStream_t stream, int quad, int no_body_fixed);

// ---------------------------------------------------------------------------------------------
// error reporting
// ---------------------------------------------------------------------------------------------

static thread_local char g_err[512] = "";

void nyx_set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

extern "C" const char *nyx_hip_last_error(void) { return g_err; }

// A refusal of one of the pure headers (run_host.h, series_host.h): its message becomes the last error, its code the return value.
static int refused(const Refusal &r) {
    nyx_set_error("%s", r.msg);
    return r.rc;
}

#define HIP_TRY(expr)                                                                      \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess) {                                                            \
            nyx_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            return NYX_HIP_RC_HIP_ERROR;                                                   \
        }                                                                                  \
    } while (0)

// Where the owners of ctx_mem.h get their memory: the device, and pinned host memory (a batch's mirror).  The codes are hipError_t.
struct DeviceMem {
    static int alloc(void **p, size_t bytes) { return (int)hipMalloc(p, bytes); }
    static void release(void *p) { (void)hipFree(p); }
    static int zero(void *p, size_t bytes) { return (int)hipMemset(p, 0, bytes); }
};
struct PinnedMem {
    static int alloc(void **p, size_t bytes) { return (int)hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static void release(void *p) { (void)hipHostFree(p); }
    static int zero(void *p, size_t bytes) { std::memset(p, 0, bytes); return 0; }
};
typedef Owned<DeviceMem> DevBuf;
static int nothing_in_flight() { return 0; }

// A device allocation of an entry's own, freed when the entry returns.
static int dev_alloc(DevBuf &b, size_t bytes) {
    if (b.ensure((int64_t)std::max<size_t>(bytes, 8), nothing_in_flight, cap_exact, PerElement{1}) == 0) return NYX_HIP_RC_OK;
    nyx_set_error("hipMalloc of %zu bytes failed", bytes);
    return NYX_HIP_RC_HIP_ERROR;
}

// ---------------------------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------------------------

struct DevArrays {  // one SoA batch resident on the device: ONE device block (arrays_block), ONE pinned host mirror => one copy each way
    DevBuf dev;
    Owned<PinnedMem> mirror;
    DevBuf stm_buf;  // [stm_buf.cap][81], allocated on first STM use
    size_t bytes = 0, state_bytes = 0;  // of the block; of its part a staged batch uploads
    // views into `dev`
    int64_t *epoch = nullptr, *step = nullptr;
    double *f[13] = {nullptr};
    int64_t *last_step = nullptr, *n_acc = nullptr, *n_rej = nullptr, *n_evals = nullptr;
    double *last_error = nullptr;
    int32_t *status = nullptr, *last_attempts = nullptr;
    double *stm() const { return stm_buf.as<double>(); }
    template <typename T> T *host(T *d) const { return (T *)(mirror.as<char>() + ((char *)d - dev.as<char>())); }
};

// Every block of device memory a context holds is an owner (ctx_mem.h) and goes with the context; the blocks that follow a batch grow
// by the owner's one rule (grow(), below).  The one exception is the mailbox block, borrowed from a pool.
struct nyx_hip_ctx {
    int device = 0;
    nyx_hip_tuning_t tune = NYX_HIP_TUNING_DEFAULT;  // config.tuning, resolved (see resolve_tuning)
    DevCfg host_cfg;
    DevBuf d_cfg;
    // opts.integration_frame: the states of a batch are centred on another body (its chain w.r.t. the integration centre)
    int swap_n_chain = 0;
    int32_t swap_seg[4] = {0, 0, 0, 0};
    double swap_sign[4] = {0.0, 0.0, 0.0, 0.0};
    DevBuf d_mom;       // scratch of the ensemble-moments reduction: [MOM_BLOCKS][MOM_N] block sums, then MOM_N results (host flavour)
    DevBuf d_stm_hist;  // NYX_HIP_FLAG_STM_TEXTBOOK: [16][12][cap] stage matrices of the attempt in flight (DevBatch.stm_hist)
    DevBuf d_swap;      // seven rows of `cap` doubles: the translated copy of a batch's Cartesian state, the forward shift's status words
    int ed_reuse_fit = 0;  // fields of stage-0 epoch data an unchained pipelined loop may carry between attempts (LDS room)
    DevBuf d_htab;
    DevBuf d_htab2;  // second gravity field
    int terms2 = 0;  // its table rows
    DevBuf d_cols2;
    DevBuf d_hyb;  // the same table in the hybrid-feed layout (devcfg.h HYB_*)
    // Run streams (DevCfg.rs_*): the table once more per column schedule - [0] SOLO, [1] PRIMARY, [2] the helpers' - with every RANGE of
    // a wave starting a sixteen-row group of its own.  Rebuilt when a schedule changes (launch() sets rs_dirty), uploaded by
    // launch() before a launch that streams the table.
    std::vector<HarmEntry> h_tab;  // host copy of the entry table (without its tail padding)
    std::vector<ColHdr> h_cols;
    std::vector<double> h_rs[3];   // (kept: the asynchronous upload reads them)
    std::vector<ColHdr> h_rs_cols[3];
    DevBuf d_rs[3], d_rs_cols[3];
    bool rs_dirty = true;
    DevBuf d_cols;
    DevBuf d_records;
    std::vector<int32_t> col_len;  // rows per column (index = c)
    int n_waves = 1;
    int forced_waves = 0;
    SchedShape shape;         // what the schedules in host_cfg were built for (launch_plan.h)
    bool sched_dirty = false; // weights changed: rebuild the schedule at the next launch
    WeightMap weights;        // per-wave column weights, calibrated on this device per workgroup shape (see calibrate())
    std::map<WKey, double> weight_spread;  // (max - min) / mean of the per-wave windows after calibration
    WKey last_key = WKey(0, 0, 0, 0);      // shape of the last launch
    DevArrays cal;                         // scratch outputs of the calibration launches
    const PredictArgs *fused_pred = nullptr;  // set around the ONE launch of a fused covariance-mapping loop (nyx_hip_predict_until): DEVICE copy of its arguments
    int forced_quad = -1;  // STM layout: -1 = by ensemble size, 0 = 64 trajectories x D3 per workgroup, 1 = quad layout (16 x 4 lanes, D1)
    double role_handicap[3] = {0.0, 0.0, 0.0};  // integrator, almanac, perturbations (harmonics-term units)
    DevArrays in, out;
    DevArrays work;            // the targeter's work block: (1 + V) n rows propagated in place (nyx_hip_target_batch), grown on demand
    DevBuf d_tgt;              // what its runs keep between the rounds (target_keep_block)
    DevBuf d_prof;             // tuning.profile, calibration: [36][8] cycle counters - rows 0-15 owner workgroup 0, 16 mailbox counts, 17-32 the first helper workgroup
    char *d_coop = nullptr;    // cooperative-mode mailboxes (mailbox_block of coop_cap): the pool's, not an owner's - see mailbox_acquire
    int64_t coop_cap = 0;
    int n_cu = 0;
    int last_coop_helpers = 0;  // helpers of the last launch (0 = solo)
    int last_helper_feed = -1;  // what their column waves walked with: 0 scalar, 1 streamed, 2 resident in LDS (-1 = no helpers)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    double last_ms = -1.0;
    // Concurrency contract (nyx_hip.h): every entry point locks `mu`, so host threads may share a context; on the DEVICE the
    // launches of one context are chained through `ev_done` (each launch waits for the previous one, whatever its stream),
    // because they share d_cfg, the cooperative-mode mailboxes and the staging blocks.  Concurrent kernels => one ctx each.
    std::recursive_mutex mu;
    hipEvent_t ev_done = nullptr;
    bool launched = false;
};
#define CTX_LOCK(ctx) std::lock_guard<std::recursive_mutex> lock_((ctx)->mu)

// Cooperative-mode mailboxes live in UNCACHED device memory (hipExtMallocWithFlags).  The blocks are pooled per process and device:
// a context borrows one at its first cooperative launch and returns it when it is destroyed; a pooled block is never freed before
// the process ends.  History: in round 3 the ~17th cooperative context of one process never finished (only behind ~90 other tests),
// the pool and the zeroing of a workgroup's LDS went in together, and the hang was gone - attributed, without a reproducer, to
// allocate / free churn of this kind of memory.  Round 4 looked for it and did NOT find it there: tools/uncached_churn.hip (the
// exchange alone: 400 allocate / free cycles x 96 pairs x 300 round trips, with and without unrelated allocator traffic, no stall)
// and tests/test_gpu_coop_contexts.py (40 cooperative contexts in one process with the pool switched OFF, debug_flags 0x100000:
// every launch completes, bit-identical results).  What the library relies on is stated in include/nyx_hip.h ("Cooperative mode");
// the pool stays because it saves an allocation and a 7 MB memset per context, not because freeing is known to be unsafe.
struct MailboxBlock { int device; void *ptr; int64_t cap; };
static std::mutex g_mailbox_mu;
static std::vector<MailboxBlock> g_mailbox_free;
static void *mailbox_acquire(int device, int64_t want_cap, int64_t *cap_out, bool pooled = true) {
    if (pooled) {
        std::lock_guard<std::mutex> lk(g_mailbox_mu);
        for (size_t k = 0; k < g_mailbox_free.size(); ++k)
            if (g_mailbox_free[k].device == device && g_mailbox_free[k].cap >= want_cap) {
                void *p = g_mailbox_free[k].ptr;
                *cap_out = g_mailbox_free[k].cap;
                g_mailbox_free.erase(g_mailbox_free.begin() + (long)k);
                return p;
            }
    }
    const int64_t cap = cap_mailbox(want_cap);
    void *p = nullptr;
    if (hipExtMallocWithFlags(&p, mailbox_block(cap).total, hipDeviceMallocUncached) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    *cap_out = cap;
    return p;
}
static void mailbox_release(int device, void *ptr, int64_t cap, bool pooled = true) {
    if (!ptr) return;
    if (!pooled) { (void)hipFree(ptr); return; }
    std::lock_guard<std::mutex> lk(g_mailbox_mu);
    g_mailbox_free.push_back(MailboxBlock{device, ptr, cap});
}

// The grow rule (Owned::ensure, ctx_mem.h) on a block of a context: what may still use the block is a launch of this context, the
// last of which ev_done marks - awaited on the host before the block is freed, at every site.  (It costs nothing: a block grows once
// per size, and hipFree waits for the device anyway.)
template <typename Mem, typename Bytes>
static hipError_t grow(nyx_hip_ctx *ctx, Owned<Mem> &b, int64_t count, int64_t (*round)(int64_t), Bytes bytes_of, bool zero = false) {
    return (hipError_t)b.ensure(count, [ctx] { return (int)(ctx->launched ? hipEventSynchronize(ctx->ev_done) : hipSuccess); }, round, bytes_of, zero);
}

// `v` on the device, in a block of its own.
template <typename T> static hipError_t upload(nyx_hip_ctx *ctx, DevBuf &b, const std::vector<T> &v) {
    if (hipError_t e = grow(ctx, b, (int64_t)v.size(), cap_exact, PerElement{sizeof(T)})) return e;
    return hipMemcpy(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
}

template <typename T> static T *part_at(char *base, const Part &p) { return (T *)(base + p.at); }

static int ensure_stm(nyx_hip_ctx *ctx, DevArrays &a, int64_t n) {  // (the STMs of the first n trajectories)
    HIP_TRY(grow(ctx, a.stm_buf, n, cap_stm, PerElement{81 * sizeof(double)}));
    return NYX_HIP_RC_OK;
}

static int ensure_arrays(nyx_hip_ctx *ctx, DevArrays &a, int64_t n, bool stats) {
    if (n <= a.dev.cap) return NYX_HIP_RC_OK;
    const auto bytes_of = [stats](int64_t cap) { return arrays_block(cap, stats).total; };
    HIP_TRY(grow(ctx, a.mirror, n, cap_batch, bytes_of));
    HIP_TRY(grow(ctx, a.dev, n, cap_batch, bytes_of, /*zero=*/true));  // (never hand the kernel recycled device memory it might read before writing)
    const auto b = arrays_block(a.dev.cap, stats);
    char *base = a.dev.as<char>();
    a.bytes = b.total;
    a.state_bytes = arrays_state_bytes(b);
    a.epoch = part_at<int64_t>(base, b[AB_EPOCH]);
    a.step = part_at<int64_t>(base, b[AB_STEP]);
    for (int k = 0; k < kStateRows; ++k) a.f[k] = part_at<double>(base, arrays_state_row(b, k));
    if (stats) {
        a.last_step = part_at<int64_t>(base, b[AB_LAST_STEP]);
        a.n_acc = part_at<int64_t>(base, b[AB_N_ACC]);
        a.n_rej = part_at<int64_t>(base, b[AB_N_REJ]);
        a.n_evals = part_at<int64_t>(base, b[AB_N_EVALS]);
        a.last_error = part_at<double>(base, b[AB_LAST_ERROR]);
        a.status = part_at<int32_t>(base, b[AB_STATUS]);
        a.last_attempts = part_at<int32_t>(base, b[AB_LAST_ATTEMPTS]);
    }
    return NYX_HIP_RC_OK;
}

extern "C" int32_t nyx_hip_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" int64_t nyx_hip_abi_sizeof(int32_t which) {
    switch (which) {
    case 0: return sizeof(nyx_hip_integ_opts_t);
    case 1: return sizeof(nyx_hip_cheby_segment_t);
    case 2: return sizeof(nyx_hip_body_t);
    case 3: return sizeof(nyx_hip_rotation_t);
    case 4: return sizeof(nyx_hip_gravity_field_t);
    case 5: return sizeof(nyx_hip_srp_t);
    case 6: return sizeof(nyx_hip_drag_t);
    case 7: return sizeof(nyx_hip_config_t);
    case 8: return sizeof(nyx_hip_states_t);
    case 9: return sizeof(nyx_hip_step_stats_t);
    case 10: return sizeof(nyx_hip_traj_t);
    case 11: return sizeof(nyx_hip_solid_tides_t);
    case 12: return sizeof(nyx_hip_predict_t);
    case 13: return sizeof(nyx_hip_predict_history_t);
    case 14: return sizeof(nyx_hip_process_noise_t);
    case 15: return sizeof(nyx_hip_tuning_t);
    default: return -1;
    }
}

// config.tuning -> the context's copy.  The process environment is consulted ONLY when NYX_HIP_TUNING_ENV is set (the A/B
// tools of this repository: tools/*.py, tools/*.sh): a library behind a C-ABI takes its switches through its config struct.
static nyx_hip_tuning_t resolve_tuning(const nyx_hip_tuning_t *t) {
    nyx_hip_tuning_t r = NYX_HIP_TUNING_DEFAULT;
    if (t) r = *t;
    if (!std::getenv("NYX_HIP_TUNING_ENV")) return r;
    auto geti = [](const char *name, int32_t &dst) { if (const char *e = std::getenv(name)) dst = (int32_t)std::strtol(e, nullptr, 0); };
    auto getd = [](const char *name, double &dst) { if (const char *e = std::getenv(name)) dst = std::atof(e); };
    int32_t cal = -1;
    geti("NYX_HIP_CALIBRATE", cal);
    if (cal == 1) r.schedule = NYX_HIP_SCHED_CALIBRATED;
    if (cal == 0) r.schedule = NYX_HIP_SCHED_MODEL;
    geti("NYX_HIP_DETERMINISTIC", r.deterministic);
    geti("NYX_HIP_COOP", r.cooperative);
    geti("NYX_HIP_PIPE", r.pipelined);
    geti("NYX_HIP_SPEC", r.chained_attempts);
    geti("NYX_HIP_ED_REUSE", r.epoch_data_reuse);
    geti("NYX_HIP_FANOUT", r.role_fanout);
    if (std::getenv("NYX_HIP_MERGE_ROLES")) r.merge_roles = 1;
    geti("NYX_HIP_STM_QUAD", r.stm_quad);
    geti("NYX_HIP_HARM_FEED", r.harmonics_feed);
    geti("NYX_HIP_COOP_COLS", r.coop_max_columns);
    geti("NYX_HIP_HELPER_RESIDENT", r.helper_resident);
    if (std::getenv("NYX_HIP_COOP_MUTE")) r.coop_mute = 1;
    if (std::getenv("NYX_HIP_PROFILE")) r.profile = 1;
    geti("NYX_HIP_DEBUG", r.debug_flags);
    getd("NYX_HIP_COOP_FRAC", r.coop_fraction);
    getd("NYX_HIP_COOP_HELPERS", r.coop_helper_ratio);
    getd("NYX_HIP_COL_FIX", r.column_start_cost);
    if (const char *e = std::getenv("NYX_HIP_ROLE_HANDICAP")) (void)std::sscanf(e, "%lf,%lf,%lf", &r.role_duties[0], &r.role_duties[1], &r.role_duties[2]);
    if (const char *e = std::getenv("NYX_HIP_AGE_WEIGHTS"))
        if (std::sscanf(e, "%lf,%lf,%lf,%lf", &r.age_weights[0], &r.age_weights[1], &r.age_weights[2], &r.age_weights[3]) == 4) r.schedule = NYX_HIP_SCHED_EXPLICIT;
    if (const char *e = std::getenv("NYX_HIP_WAVE_WEIGHTS")) {
        const char *q = e;
        for (int w = 0; w < 16 && *q; ++w) { r.wave_weights[w] = std::strtod(q, (char **)&q); if (*q == ',') ++q; }
        r.schedule = NYX_HIP_SCHED_EXPLICIT;
    }
    return r;
}

// What the launch planner (launch_plan.h) reads of a context.
static PlanInputs plan_inputs(const nyx_hip_ctx *ctx) {
    return PlanInputs{ctx->tune, ctx->col_len, ctx->role_handicap, ctx->terms2, ctx->ed_reuse_fit, ctx->n_cu, ctx->forced_waves, ctx->forced_quad, ctx->weights};
}

extern "C" int32_t nyx_hip_ctx_set_column_waves(nyx_hip_ctx *ctx, int32_t waves) {
    if (!ctx || waves < 0 || waves > DEV_MAX_WAVES) return NYX_HIP_RC_BAD_ARG;
    CTX_LOCK(ctx);
    ctx->forced_waves = waves;
    return NYX_HIP_RC_OK;
}

extern "C" int32_t nyx_hip_last_coop_helpers(nyx_hip_ctx *ctx) { return ctx ? ctx->last_coop_helpers : 0; }

// Introspection (tests, tools): the feed of the helpers' column walk in the last launch - 0 scalar, 1 streamed, 2 resident in LDS;
// -1 when it had no helpers.
extern "C" int32_t nyx_hip_debug_helper_feed(nyx_hip_ctx *ctx) { return ctx ? ctx->last_helper_feed : -1; }

// The first `count` column weights of the last launch's workgroup shape (WeightMap), then the spread (max - min) / mean of the
// per-wave windows measured when they were calibrated (-1 = structural default weights, never calibrated).
static int32_t last_weights(nyx_hip_ctx *ctx, double *out, int count) {
    if (!ctx || !out) return NYX_HIP_RC_BAD_ARG;
    CTX_LOCK(ctx);
    const auto it = ctx->weights.find(ctx->last_key);
    for (int w = 0; w < count; ++w) out[w] = it != ctx->weights.end() ? it->second[w] : 0.0;
    const auto sp = ctx->weight_spread.find(ctx->last_key);
    out[count] = sp != ctx->weight_spread.end() ? sp->second : -1.0;
    return NYX_HIP_RC_OK;
}

// Introspection: the speed weights and the spread, out[17].
extern "C" int32_t nyx_hip_debug_weights(nyx_hip_ctx *ctx, double *out) { return last_weights(ctx, out, DEV_MAX_WAVES); }

// Shape of the last launch's workgroups (tools): waves, pipelined loop, carried epoch-data fields, chained attempts, ephemeris
// records in LDS, their size in doubles, almanac waves, LDS bytes of the plain kernel.
extern "C" int32_t nyx_hip_debug_layout(nyx_hip_ctx *ctx, int32_t *out) {
    if (!ctx || !out) return NYX_HIP_RC_BAD_ARG;
    CTX_LOCK(ctx);
    const DevCfg &dc = ctx->host_cfg;
    out[0] = dc.n_waves; out[1] = dc.pipe; out[2] = dc.ed_reuse; out[3] = dc.spec; out[4] = dc.rec_in_lds; out[5] = dc.rec_doubles;
    out[6] = dc.n_alm;
    out[7] = (int32_t)nyx_kernel_lds_bytes(DEV_MAX_WAVES, dc.rec_in_lds ? dc.rec_doubles : 0, 0, dc.ed_reuse);
    return NYX_HIP_RC_OK;
}

// Roles of the last launch's workgroup shape (tools): out[w] = role_kind, out[16 + w] = role_mask of wave w.
extern "C" int32_t nyx_hip_debug_roles(nyx_hip_ctx *ctx, int32_t *out) {
    if (!ctx || !out) return NYX_HIP_RC_BAD_ARG;
    CTX_LOCK(ctx);
    const DevCfg &dc = ctx->host_cfg;
    for (int w = 0; w < DEV_MAX_WAVES; ++w) { out[w] = dc.role_kind[w]; out[DEV_MAX_WAVES + w] = dc.role_mask[w]; }
    return NYX_HIP_RC_OK;
}

// Calibration of the column weights: 1 = on the device, once per workgroup shape, 0 = the model's weights (tuning.schedule).
extern "C" int32_t nyx_hip_debug_set_calibration(nyx_hip_ctx *ctx, int32_t mode) {
    if (!ctx || mode < 0 || mode > 1) return NYX_HIP_RC_BAD_ARG;
    CTX_LOCK(ctx);
    ctx->tune.schedule = mode ? NYX_HIP_SCHED_CALIBRATED : NYX_HIP_SCHED_MODEL;
    return NYX_HIP_RC_OK;
}

// The launch-time part of the tuning (cooperative mode, determinism, schedule kind and explicit weights, helper ratio / share /
// mute, profiling) may be changed between launches; the create-time part (stage loop, role layout, feed) is fixed with the context.
extern "C" int32_t nyx_hip_ctx_set_tuning(nyx_hip_ctx *ctx, const nyx_hip_tuning_t *t) {
    if (!ctx) return NYX_HIP_RC_BAD_ARG;
    CTX_LOCK(ctx);
    const nyx_hip_tuning_t n = resolve_tuning(t), &o = ctx->tune;
    if (n.pipelined != o.pipelined || n.chained_attempts != o.chained_attempts || n.epoch_data_reuse != o.epoch_data_reuse ||
        n.role_fanout != o.role_fanout || n.merge_roles != o.merge_roles || n.harmonics_feed != o.harmonics_feed ||
        n.debug_flags != o.debug_flags || std::memcmp(n.role_duties, o.role_duties, sizeof n.role_duties) != 0) {
        nyx_set_error("nyx_hip_ctx_set_tuning: stage loop, role layout, feed and debug switches are fixed at nyx_hip_ctx_create");
        return NYX_HIP_RC_BAD_ARG;
    }
    ctx->tune = n;
    // the helper share the schedules are built for follows the new request (auto: 0.30 until a cooperative launch derives it from
    // its helper / owner ratio); the rebuilt descriptor is uploaded by the next launch (sched_dirty)
    ctx->host_cfg.coop_frac = n.coop_fraction > 0.0 ? std::min(0.9, std::max(0.05, n.coop_fraction)) : 0.30;
    ctx->weights.clear();
    ctx->weight_spread.clear();
    ctx->sched_dirty = true;
    return NYX_HIP_RC_OK;
}

// Speed weights [0..16), duties [16..32) and the window spread [32] of the last launch's workgroup shape (tools).
extern "C" int32_t nyx_hip_debug_schedule_weights(nyx_hip_ctx *ctx, double *out) { return last_weights(ctx, out, 2 * DEV_MAX_WAVES); }

// Table rows wave w walks under `sd` (a column outside the table counts nothing).
static int rows_of(const nyx_hip_ctx *ctx, const DevSched &sd, int w) {
    int rows = 0;
    for (int q = 0; q < sd.n_ranges[w]; ++q)
        for (int c = sd.range_c0[w][q]; c < sd.range_c0[w][q] + sd.range_cnt[w][q]; ++c) rows += (c >= 0 && c < (int)ctx->col_len.size()) ? ctx->col_len[c] : 0;
    return rows;
}

// Table rows each wave walks under schedule `sched` (DEV_SCHED_*) of the current descriptor, and the role duties the water-filling
// charged (integrator, almanac, perturbations; harmonics-term units): what tools/tune_schedule.py turns measured windows into weights with.
extern "C" int32_t nyx_hip_debug_schedule_rows(nyx_hip_ctx *ctx, int32_t sched, int32_t *rows16, double *duties3) {
    if (!ctx || !rows16 || sched < 0 || sched >= DEV_N_SCHED) return NYX_HIP_RC_BAD_ARG;
    CTX_LOCK(ctx);
    for (int w = 0; w < DEV_MAX_WAVES; ++w) rows16[w] = rows_of(ctx, ctx->host_cfg.sched[sched], w);
    if (duties3) for (int k = 0; k < 3; ++k) duties3[k] = ctx->role_handicap[k];
    return NYX_HIP_RC_OK;
}

// Test / tuning hook: STM layout of the following launches (-1 = by ensemble size, 0 = D3 64-lane, 1 = quad).
extern "C" int32_t nyx_hip_debug_set_stm_layout(nyx_hip_ctx *ctx, int32_t quad) {
    if (!ctx || quad < -1 || quad > 1) return NYX_HIP_RC_BAD_ARG;
    CTX_LOCK(ctx);
    ctx->forced_quad = quad;
    return NYX_HIP_RC_OK;
}

// The time of the last timed kernel (ev0 -> ev1) into ctx->last_ms: -1 when it cannot be read.
static double read_kernel_ms(nyx_hip_ctx *ctx) {
    float ms = 0.f;
    ctx->last_ms = (hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1) == hipSuccess) ? ms : -1.0;
    return ctx->last_ms;
}

extern "C" double nyx_hip_last_kernel_ms(nyx_hip_ctx *ctx) {
    if (!ctx || !ctx->ev1) return -1.0;
    CTX_LOCK(ctx);
    if (hipEventSynchronize(ctx->ev1) != hipSuccess) return -1.0;
    return read_kernel_ms(ctx);
}

// Cycle accounting of workgroup 0 of the last launch (NYX_HIP_PROFILE=1): out[17][8], see the kernel (row 16: mailbox counters).
extern "C" int32_t nyx_hip_debug_profile_helper(nyx_hip_ctx *ctx, int64_t *out /* [19][8] */) {
    if (!ctx || !ctx->d_prof.p) return NYX_HIP_RC_BAD_ARG;
    if (hipMemcpy(out, ctx->d_prof.as<int64_t>() + 17 * 8, 19 * 8 * sizeof(int64_t), hipMemcpyDeviceToHost) != hipSuccess) return NYX_HIP_RC_HIP_ERROR;  // (row 16 of `out` = row 33: the owner's latency loop; rows 17-18 = the integrator's stage in pieces)
    return NYX_HIP_RC_OK;
}
extern "C" int32_t nyx_hip_debug_profile(nyx_hip_ctx *ctx, int64_t *out) {
    if (!ctx || !ctx->d_prof.p) return NYX_HIP_RC_BAD_ARG;
    if (hipMemcpy(out, ctx->d_prof.p, 17 * 8 * sizeof(int64_t), hipMemcpyDeviceToHost) != hipSuccess) return NYX_HIP_RC_HIP_ERROR;
    return NYX_HIP_RC_OK;
}

// (the context's blocks are owners: `delete` frees them, on the context's device)
extern "C" void nyx_hip_ctx_destroy(nyx_hip_ctx *ctx) {
    if (!ctx) return;
    hipSetDevice(ctx->device);
    mailbox_release(ctx->device, ctx->d_coop, ctx->coop_cap, !(ctx->tune.debug_flags & 0x100000));
    if (ctx->ev0) hipEventDestroy(ctx->ev0);
    if (ctx->ev1) hipEventDestroy(ctx->ev1);
    if (ctx->ev_done) hipEventDestroy(ctx->ev_done);
    delete ctx;
}

extern "C" int32_t nyx_hip_ctx_create(const nyx_hip_config_t *cfg, int32_t device, nyx_hip_ctx **out) {
    if (!cfg || !out) { nyx_set_error("null argument"); return NYX_HIP_RC_BAD_ARG; }
    *out = nullptr;
    if (cfg->abi_version != NYX_HIP_ABI_VERSION) { nyx_set_error("ABI version mismatch"); return NYX_HIP_RC_BAD_ARG; }
    const nyx_hip_tuning_t tune = resolve_tuning(cfg->tuning);
    CtxBuild b;  // validation, descriptor, records and tables (ctx_build.h): nothing touches a device before it has passed
    if (build_context(*cfg, tune, nyx_kernel_lds_bytes, b) != NYX_HIP_RC_OK) { nyx_set_error("%s", b.error.c_str()); return b.rc; }
    if (nyx_hip_device_count() <= device || device < 0) { nyx_set_error("no HIP device %d", device); return NYX_HIP_RC_NO_DEVICE; }
    HIP_TRY(hipSetDevice(device));

    // the owner of a context under construction: every failure below (HIP_TRY included) frees what was allocated so far
    std::unique_ptr<nyx_hip_ctx, void (*)(nyx_hip_ctx *)> ctx(new nyx_hip_ctx(), nyx_hip_ctx_destroy);
    ctx->device = device;
    ctx->tune = tune;
    DevCfg &dc = ctx->host_cfg;
    std::memcpy(&dc, &b.dc, sizeof dc);
    ctx->swap_n_chain = b.swap_n_chain;
    std::memcpy(ctx->swap_seg, b.swap_seg, sizeof b.swap_seg);
    std::memcpy(ctx->swap_sign, b.swap_sign, sizeof b.swap_sign);
    std::memcpy(ctx->role_handicap, b.role_handicap, sizeof b.role_handicap);
    ctx->terms2 = b.terms2;
    ctx->ed_reuse_fit = b.ed_reuse_fit;
    ctx->col_len = b.col_len;
    ctx->h_tab = b.tab;
    ctx->h_cols = b.cols;
    {
        hipDeviceProp_t prop;
        ctx->n_cu = (hipGetDeviceProperties(&prop, device) == hipSuccess) ? prop.multiProcessorCount : 0;
    }
    plan_first_schedule(plan_inputs(ctx.get()), dc, ctx->shape, b.harm_feed);

    // ---- upload
    std::vector<HarmEntry> &tab = b.tab, &tab2 = b.tab2;
    if (!tab.empty()) {
        std::vector<double> hyb;
        int64_t vec_off = 0;
        build_hybrid(tab, hyb, vec_off);
        HIP_TRY(upload(ctx.get(), ctx->d_hyb, hyb));
        dc.hyb = (uint64_t)ctx->d_hyb.p;
        dc.hyb_v = (uint64_t)(ctx->d_hyb.as<double>() + vec_off);
    }
    if (!tab2.empty()) {
        tab2.resize(tab2.size() + 4 * HARM_BATCH, HarmEntry{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0});
        HIP_TRY(upload(ctx.get(), ctx->d_htab2, tab2));
        HIP_TRY(upload(ctx.get(), ctx->d_cols2, b.cols2));
        dc.htab2 = (uint64_t)ctx->d_htab2.p;
        dc.cols2 = (uint64_t)ctx->d_cols2.p;
    }
    HIP_TRY(upload(ctx.get(), ctx->d_cfg, std::vector<DevCfg>(1, dc)));  // (the descriptor: a table of one)
    if (!tab.empty()) {
        tab.resize(tab.size() + 4 * HARM_BATCH, HarmEntry{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0});  // the kernel touches a few batches ahead
        HIP_TRY(upload(ctx.get(), ctx->d_htab, tab));
        HIP_TRY(upload(ctx.get(), ctx->d_cols, b.cols));
    }
    HIP_TRY(upload(ctx.get(), ctx->d_records, b.records));
    HIP_TRY(hipEventCreate(&ctx->ev0));
    HIP_TRY(hipEventCreate(&ctx->ev1));
    HIP_TRY(hipEventCreateWithFlags(&ctx->ev_done, hipEventDisableTiming));
    *out = ctx.release();
    return NYX_HIP_RC_OK;
}

// ---------------------------------------------------------------------------------------------
// propagate
// ---------------------------------------------------------------------------------------------

static int launch(nyx_hip_ctx *ctx, const LaunchReq &r);

// Device views of a DevArrays block (outputs + stats).
static void views_of(DevArrays &d, int64_t n, bool stm, nyx_hip_states_t &so, nyx_hip_step_stats_t &ss) {
    std::memset(&so, 0, sizeof so);
    so.n = n; so.epoch_ns = d.epoch;
    for (int k = 0; k < kStateRows; ++k) so.*kStateRow[k].s = d.f[k];
    so.step_ns = d.step;
    so.stm = stm ? d.stm() : nullptr;
    ss = {d.status, d.last_step, d.last_error, d.last_attempts, d.n_acc, d.n_rej, d.n_evals};
}

// On-device calibration of the column schedule of the shape the NEXT launch of `in` will have: up to four short launches of the
// workload's own first steps (30 steps; 4 with the STM) into scratch outputs with the in-kernel cycle accounting on, each fitted by
// calibration_fit (launch_plan.h), until the windows agree.  Kept for the life of the context: its launches are deterministic.
static int calibrate(nyx_hip_ctx *ctx, const nyx_hip_states_t *in, hipStream_t stream, bool backward = false) {
    const bool stm = (ctx->host_cfg.flags & NYX_HIP_FLAG_STM) != 0;
    const int64_t n = in->n;
    if (int rc = ensure_arrays(ctx, ctx->cal, n, true)) return rc;
    if (int rc = stm ? ensure_stm(ctx, ctx->cal, n) : NYX_HIP_RC_OK) return rc;
    nyx_hip_states_t so;
    nyx_hip_step_stats_t ss;
    views_of(ctx->cal, n, stm, so, ss);
    LaunchReq r;
    r.in = in; r.out = &so; r.stats = &ss; r.stream = stream; r.calibrating = true;
    r.duration_ns = (backward ? -1 : 1) * (stm ? 4 : 30) * ctx->host_cfg.init_step_ns;  // the direction of the real request: the ephemerides may end either way
    std::vector<int32_t> cal_status((size_t)n);
    CalibrationFit fit;  // the last usable one
    WKey key(0, 0, 0, 0);
    std::vector<int64_t> prof(17 * 8);
    for (int it = 0; it < 4; ++it) {
        if (fit.usable) { ctx->weights[key] = fit.w; ctx->sched_dirty = true; }
        if (int rc = launch(ctx, r)) return rc;
        HIP_TRY(hipStreamSynchronize(stream));
        HIP_TRY(hipMemcpy(prof.data(), ctx->d_prof.p, prof.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
        if (ss.status) {  // lanes that died early produce garbage cycle counts: keep the model's weights then
            HIP_TRY(hipMemcpy(cal_status.data(), ss.status, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
            bool bad = false;
            for (int64_t q = 0; q < n && !bad; ++q) bad = cal_status[(size_t)q] != NYX_HIP_OK;
            if (bad) { fit.usable = false; ctx->weights.erase(ctx->last_key); ctx->sched_dirty = true; break; }
        }
        key = ctx->last_key;
        const DevSched &sd = ctx->host_cfg.sched[std::get<3>(key) >= 0 ? DEV_SCHED_PRIMARY : DEV_SCHED_SOLO];
        const CalibrationFit f = calibration_fit(prof.data(), sd, ctx->col_len, std::get<0>(key), fit.usable ? &fit.w : nullptr);
        if (!f.usable) break;
        fit = f;
        if (it > 0 && fit.spread < 0.08) break;
    }
    if (fit.usable) {
        ctx->weights[key] = fit.w;
        ctx->weight_spread[key] = fit.spread;
        ctx->sched_dirty = true;
    }
    return NYX_HIP_RC_OK;
}

// ---- the steps of a launch (launch_here, below), in its order

// The launch-shape dependent parts of the descriptor, after the plan (waves per workgroup, column schedules and cooperative mode:
// launch_plan.h): whether the ephemeris records fit in LDS next to this layout's buffers (the quad layout is smaller than the D3 one).
static int refresh_descriptor(nyx_hip_ctx *ctx, const LaunchPlan &plan, hipStream_t stream) {
    const int kind = (ctx->host_cfg.flags & NYX_HIP_FLAG_STM) ? (plan.quad ? 2 : 1) : 0;
    const int rd = ctx->host_cfg.rec_doubles;  // (after the schedule: chained attempts give the carried epoch data's LDS back)
    const int want_rec = records_fit_lds(nyx_kernel_lds_bytes, rd, DEV_MAX_WAVES, kind, kind == 0 ? ctx->host_cfg.ed_reuse : 0) ? 1 : 0;
    const bool dirty = plan.rebuilt || want_rec != ctx->host_cfg.rec_in_lds;
    ctx->host_cfg.rec_in_lds = want_rec;
    if (plan.rebuilt) ctx->rs_dirty = true;  // (the run streams follow the schedules)
    if (dirty) HIP_TRY(hipMemcpyAsync(ctx->d_cfg.p, &ctx->host_cfg, sizeof(DevCfg), hipMemcpyHostToDevice, stream));
    return NYX_HIP_RC_OK;
}

// NYX_HIP_FLAG_STM_TEXTBOOK: the stage matrices of the attempt in flight.
static int bind_textbook_history(nyx_hip_ctx *ctx, int64_t n, DevBatch &bt) {
    if (!(ctx->host_cfg.flags & NYX_HIP_FLAG_STM_TEXTBOOK)) return NYX_HIP_RC_OK;
    HIP_TRY(grow(ctx, ctx->d_stm_hist, n, cap_stm_hist, PerElement{DEV_MAX_STAGES * 12 * sizeof(double)}));
    bt.stm_hist = ctx->d_stm_hist.as<double>();
    bt.stm_hist_stride = ctx->d_stm_hist.cap;
    return NYX_HIP_RC_OK;
}

// Cooperative mode (plan.coop): helper workgroups on the idle CUs take over a share of the harmonics columns
// (propagate_kernel.hip).  Owners and helpers that talk to each other get block indices that agree modulo 8 (round-robin XCD
// dispatch: same L2).  Their mailboxes: borrowed from the pool, grown, cleared and bound (mailbox_block).
static int bind_mailboxes(nyx_hip_ctx *ctx, const CoopPlan &cp, int32_t staged_groups, DevBatch &bt, hipStream_t stream) {
    ctx->last_coop_helpers = 0;
    ctx->last_helper_feed = -1;
    if (!cp.run) return NYX_HIP_RC_OK;
    const bool pooled = !(ctx->tune.debug_flags & 0x100000);
    if (ctx->coop_cap < cp.boxes || ctx->coop_cap < cp.answers) {
        // the block goes back to the process-wide pool, where another context (another host thread) may take and clear it
        // at once: not before every launch of THIS context that uses it has finished (the device entry points are asynchronous)
        if (ctx->d_coop && ctx->launched) HIP_TRY(hipEventSynchronize(ctx->ev_done));
        mailbox_release(ctx->device, ctx->d_coop, ctx->coop_cap, pooled);
        ctx->d_coop = nullptr;
        ctx->coop_cap = 0;
        // uncached device memory: the mailboxes are coherent across the XCDs' L2s without any cache
        // write-back / invalidate in the kernel (those would also flush the harmonics table out of L2)
        int64_t got = 0;
        ctx->d_coop = (char *)mailbox_acquire(ctx->device, std::max<int64_t>({cp.boxes, cp.answers, 256}), &got, pooled);
        if (ctx->d_coop) ctx->coop_cap = got;  // (else: no such memory here, every workgroup works alone)
    }
    if (!ctx->d_coop) return NYX_HIP_RC_OK;
    const auto mb = mailbox_block(ctx->coop_cap);
    // (only what this launch touches: its mailboxes, the scan words, and its answer blocks)
    HIP_TRY(hipMemsetAsync(ctx->d_coop, 0, (size_t)cp.boxes * sizeof(CoopBox), stream));
    HIP_TRY(hipMemsetAsync(ctx->d_coop + mb[MB_POSTED].at, 0, mb[MB_ANSWERS].at - mb[MB_POSTED].at, stream));
    CoopOut *out2 = part_at<CoopOut>(ctx->d_coop, mb[MB_ANSWERS]);
    if (cp.answers) HIP_TRY(hipMemsetAsync(out2, 0, (size_t)cp.answers * sizeof(CoopOut), stream));
    bt.coop_out2 = cp.answers ? out2 : nullptr;
    bt.coop_fan = cp.fan ? 1 : 0;
    bt.coop_helpers = (int32_t)cp.helpers; bt.coop_base = (int32_t)cp.base; bt.coop_box = part_at<CoopBox>(ctx->d_coop, mb[MB_BOXES]);
    bt.coop_posted = part_at<uint32_t>(ctx->d_coop, mb[MB_POSTED]);
    bt.coop_claimed = part_at<uint32_t>(ctx->d_coop, mb[MB_CLAIMED]);
    bt.coop_finished = part_at<uint32_t>(ctx->d_coop, mb[MB_FINISHED]);
    bt.coop_sets = (int32_t)((cp.n_own + 15) / 16);
    bt.coop_parts = cp.parts;
    bt.coop_mute = ctx->tune.coop_mute ? 1 : 0;  // (bit 1, the retired speculative fetch of helper_body, stays clear)
    ctx->last_coop_helpers = (int)cp.helpers;
    // the resident feed: this launch's LDS holds the staged rows behind the helper's carve (select_helper_feed said that they fit)
    bt.coop_stage = (int32_t)helper_stage_bytes(staged_groups);
    ctx->last_helper_feed = staged_groups > 0 ? 2 : ((ctx->host_cfg.harm_feed & 2) ? 1 : 0);
    return NYX_HIP_RC_OK;
}

// Workgroups that stream the table walk run streams: one per schedule, every range of a wave at the head of a sixteen-row group
// (DevCfg.rs_*, build_run_stream); rebuilt and uploaded when the schedules have changed.
static int upload_run_streams(nyx_hip_ctx *ctx, hipStream_t stream) {
    DevCfg &dc = ctx->host_cfg;
    if (ctx->h_tab.empty() || (dc.harm_feed == 0 && dc.hres_groups == 0) || (dc.flags & NYX_HIP_FLAG_STM) || !ctx->rs_dirty) return NYX_HIP_RC_OK;
    for (int k = 0; k < 3; ++k) {
        // (the helpers' stream: walked from global memory by the streamed feed, staged from it by the resident one)
        const bool used = k == 0 ? (dc.harm_feed & 1) != 0 : (dc.coop_ok != 0 && (k == 1 ? (dc.harm_feed & 1) != 0 : ((dc.harm_feed & 2) != 0 || dc.hres_groups > 0)));
        dc.rs_hyb[k] = 0;
        if (!used) continue;
        std::vector<double> &rs = ctx->h_rs[k];
        std::vector<ColHdr> &rs_cols = ctx->h_rs_cols[k];
        int64_t vec_off = 0;
        if (k == 0) build_run_stream(ctx->h_cols, ctx->h_tab, dc.sched, {DEV_SCHED_SOLO}, rs, vec_off, rs_cols);
        else if (k == 1) build_run_stream(ctx->h_cols, ctx->h_tab, dc.sched, {DEV_SCHED_PRIMARY}, rs, vec_off, rs_cols);
        else build_run_stream(ctx->h_cols, ctx->h_tab, dc.sched, {DEV_SCHED_HELPER, DEV_SCHED_HELPER2}, rs, vec_off, rs_cols);
        HIP_TRY(grow(ctx, ctx->d_rs[k], (int64_t)rs.size(), cap_exact, PerElement{sizeof(double)}));
        HIP_TRY(grow(ctx, ctx->d_rs_cols[k], (int64_t)rs_cols.size(), cap_exact, PerElement{sizeof(ColHdr)}));
        HIP_TRY(hipMemcpyAsync(ctx->d_rs[k].p, rs.data(), rs.size() * sizeof(double), hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemcpyAsync(ctx->d_rs_cols[k].p, rs_cols.data(), rs_cols.size() * sizeof(ColHdr), hipMemcpyHostToDevice, stream));
        dc.rs_hyb[k] = (uint64_t)ctx->d_rs[k].p;
        dc.rs_hyb_v[k] = (uint64_t)(ctx->d_rs[k].as<double>() + vec_off);
        dc.rs_cols[k] = (uint64_t)ctx->d_rs_cols[k].p;
    }
    ctx->rs_dirty = false;
    HIP_TRY(hipMemcpyAsync(ctx->d_cfg.p, &dc, sizeof(DevCfg), hipMemcpyHostToDevice, stream));
    return NYX_HIP_RC_OK;
}

// tuning.profile, a calibration launch: the cycle counters, cleared.
static int bind_profile_block(nyx_hip_ctx *ctx, bool calibrating, DevBatch &bt, hipStream_t stream) {
    if (!ctx->tune.profile && !calibrating) return NYX_HIP_RC_OK;
    HIP_TRY(grow(ctx, ctx->d_prof, 36 * 8, cap_exact, PerElement{sizeof(int64_t)}));
    HIP_TRY(hipMemsetAsync(ctx->d_prof.p, 0, 36 * 8 * sizeof(int64_t), stream));
    bt.prof = ctx->d_prof.as<int64_t>();
    return NYX_HIP_RC_OK;
}

// The kernel between its events.
static int launch_kernel(nyx_hip_ctx *ctx, const LaunchPlan &plan, const DevBatch &bt, bool timed, hipStream_t stream) {
    const DevCfg &dc = ctx->host_cfg;
    if (timed) HIP_TRY(hipEventRecord(ctx->ev0, stream));
    // (the LDS staging of the ephemeris records was decided at ctx_create for the D3 layout; the quad layout is smaller)
    HIP_TRY(nyx_launch_propagate(bt, ctx->d_cfg.as<DevCfg>(), ctx->d_htab.as<HarmEntry>(), ctx->d_cols.as<ColHdr>(), ctx->d_records.as<double>(), plan.n_waves,
                                 dc.rec_in_lds ? dc.rec_doubles : 0, dc.ed_reuse, stream, plan.quad ? 1 : 0,
                                 (!dc.has_grav && !dc.has_drag && !dc.has_tides && !dc.has_grav2) ? 1 : 0));
    if (timed) HIP_TRY(hipEventRecord(ctx->ev1, stream));
    HIP_TRY(hipEventRecord(ctx->ev_done, stream));
    ctx->launched = true;
    return NYX_HIP_RC_OK;
}

// One launch, in the frame the context integrates in.
static int launch_here(nyx_hip_ctx *ctx, const LaunchReq &r) {
    CTX_LOCK(ctx);
    const hipStream_t stream = (hipStream_t)r.stream;
    const nyx_hip_states_t *in = r.in;
    if (ctx->launched) HIP_TRY(hipStreamWaitEvent(stream, ctx->ev_done, 0));  // one launch of a context at a time on the device
    const LaunchPlan plan = plan_launch(plan_inputs(ctx), ctx->host_cfg, ctx->shape, in->n, ctx->sched_dirty);
    ctx->sched_dirty = false;
    if (int rc = refresh_descriptor(ctx, plan, stream)) return rc;
    BoundBatch b = bind_batch(r, (ctx->host_cfg.flags & NYX_HIP_FLAG_STM) != 0, ctx->fused_pred);
    if (b.rc != NYX_HIP_RC_OK) { nyx_set_error("%s", b.error); return b.rc; }
    if (int rc = bind_textbook_history(ctx, in->n, b.bt)) return rc;
    if (int rc = bind_mailboxes(ctx, plan.coop, plan.staged_groups, b.bt, stream)) return rc;
    if (int rc = upload_run_streams(ctx, stream)) return rc;
    // (what helper_body checks before it walks from LDS, checked here too: the report says what ran, not what was planned)
    if (ctx->last_helper_feed == 2 && !(ctx->host_cfg.rs_hyb[2] != 0 && ctx->host_cfg.hres_groups == plan.staged_groups && b.bt.coop_stage >= helper_stage_bytes(ctx->host_cfg.hres_groups)))
        ctx->last_helper_feed = (ctx->host_cfg.harm_feed & 2) ? 1 : 0;
    // the column weights of this launch's workgroup shape: measured once per context (see calibrate())
    const WKey key = weight_key(ctx->host_cfg, plan.n_waves, plan.quad, b.bt.coop_helpers > 0);
    ctx->last_key = key;
    const int64_t span = r.use_end ? INT64_MAX : (r.duration_ns < 0 ? -r.duration_ns : r.duration_ns);
    if (calibrates_first(plan_inputs(ctx), ctx->host_cfg, key, plan.n_waves, in->n, /*min_n=*/64, !r.calibrating && !r.traj && !r.dur_ns && !r.ev, span, /*min_steps=*/100)) {
        if (int rc = calibrate(ctx, in, stream, !r.use_end && r.duration_ns < 0)) return rc;
        return launch_here(ctx, r);
    }
    if (int rc = bind_profile_block(ctx, r.calibrating, b.bt, stream)) return rc;
    return launch_kernel(ctx, plan, b.bt, r.timed, stream);
}

static int launch(nyx_hip_ctx *ctx, const LaunchReq &r) {
    CTX_LOCK(ctx);
    if (ctx->swap_n_chain == 0 || r.calibrating) return launch_here(ctx, r);
    // opts.integration_frame (instance.rs:117-142, 211-220): translate a COPY of the Cartesian state into the integration frame
    // at the start epochs, propagate that, translate the final states back at their own epochs
    // Dense output and per-trajectory durations go through (round 4).  What the reference's `Traj` holds then (instance.rs:297-326
    // around :117-142): the START state as it was handed in - its own frame -, every published state in the INTEGRATION frame (the
    // channel is fed inside the loop, the translation back is applied to the returned state only, :211-220).  Reproduced as is:
    // entry 0 of the dense output is rewritten with the caller's state below.  The event search is still refused: there the
    // reference returns from inside the loop without translating back (:243-250) - a state whose frame depends on how the run ended.
    if (r.ev) {
        nyx_set_error("integration-frame swap: the event search does not take states of another frame");
        return NYX_HIP_RC_UNSUPPORTED;
    }
    const hipStream_t stream = (hipStream_t)r.stream;
    const nyx_hip_states_t *in = r.in, *out = r.out;
    if (ctx->launched) HIP_TRY(hipStreamWaitEvent(stream, ctx->ev_done, 0));  // (the copy below is shared by the launches of this context)
    HIP_TRY(grow(ctx, ctx->d_swap, in->n, cap_exact, PerElement{7 * sizeof(double)}));  // (row 6: the forward shift's status words)
    double *swap = ctx->d_swap.as<double>();
    const size_t swap_row = (size_t)ctx->d_swap.cap;
    nyx_hip_states_t in2 = *in;
    for (int q = 0; q < kCartRows; ++q) {
        double *row = in2.*kStateRow[q].s = swap + (size_t)q * swap_row;
        HIP_TRY(hipMemcpyAsync(row, in->*kStateRow[q].s, (size_t)in->n * sizeof(double), hipMemcpyDeviceToDevice, stream));
    }
    // a start epoch outside the swap body's ephemeris gives a clamped, i.e. WRONG, translation: its status is kept aside and
    // merged into the run's status by the back-translation (the propagation launch rewrites the status array in between)
    int32_t *fwd_status = (int32_t *)(swap + 6 * swap_row);
    HIP_TRY(hipMemsetAsync(fwd_status, 0, (size_t)in->n * sizeof(int32_t), stream));
    HIP_TRY(nyx_launch_frame_shift(ctx->d_cfg.as<DevCfg>(), ctx->d_records.as<double>(), ctx->swap_seg, ctx->swap_sign, ctx->swap_n_chain, in->n, in->epoch_ns,
                                   in2.x_km, in2.y_km, in2.z_km, in2.vx_km_s, in2.vy_km_s, in2.vz_km_s, +1.0, fwd_status, nullptr, r.dur_ns, stream));
    LaunchReq r2 = r;
    r2.in = &in2;
    if (int rc = launch_here(ctx, r2)) return rc;
    if (r.traj && r.traj->capacity > 0)  // entry 0 (step-major: the first n elements of every array) = the state in the caller's frame
        for (int q = 0; q < kCartRows; ++q)
            if (double *dst = r.traj->*kTrajRow[q]) HIP_TRY(hipMemcpyAsync(dst, in->*kStateRow[q].s, (size_t)in->n * sizeof(double), hipMemcpyDeviceToDevice, stream));
    HIP_TRY(nyx_launch_frame_shift(ctx->d_cfg.as<DevCfg>(), ctx->d_records.as<double>(), ctx->swap_seg, ctx->swap_sign, ctx->swap_n_chain, in->n, out->epoch_ns,
                                   out->x_km, out->y_km, out->z_km, out->vx_km_s, out->vy_km_s, out->vz_km_s, -1.0, r.stats ? r.stats->status : nullptr,
                                   fwd_status, r.dur_ns, stream));
    HIP_TRY(hipEventRecord(ctx->ev_done, stream));
    return NYX_HIP_RC_OK;
}

// The device entry points: the caller's device arrays, on the caller's stream.
static int propagate_device(nyx_hip_ctx *ctx, const nyx_hip_states_t *in, int64_t duration_ns, nyx_hip_states_t *out,
                            nyx_hip_step_stats_t *stats, const nyx_hip_traj_t *traj, void *hip_stream) {
    if (Refusal r = check_states(in, "in")) return refused(r);
    if (Refusal r = check_states(out, "out")) return refused(r);
    if (in->n == 0) return NYX_HIP_RC_OK;
    CTX_LOCK(ctx);
    HIP_TRY(hipSetDevice(ctx->device));
    LaunchReq r;
    r.in = in; r.out = out; r.stats = stats; r.duration_ns = duration_ns; r.traj = traj; r.stream = hip_stream; r.timed = true;
    return launch(ctx, r);
}

extern "C" int32_t nyx_hip_propagate_batch_device(nyx_hip_ctx *ctx, const nyx_hip_states_t *in, int64_t duration_ns,
                                                  nyx_hip_states_t *out, nyx_hip_step_stats_t *stats, void *hip_stream) {
    if (!ctx) { nyx_set_error("null ctx"); return NYX_HIP_RC_BAD_ARG; }
    return propagate_device(ctx, in, duration_ns, out, stats, nullptr, hip_stream);
}

extern "C" int32_t nyx_hip_propagate_batch_with_traj_device(nyx_hip_ctx *ctx, const nyx_hip_states_t *in, int64_t duration_ns,
                                                            nyx_hip_states_t *out, nyx_hip_step_stats_t *stats, nyx_hip_traj_t *traj,
                                                            void *hip_stream) {
    if (!ctx || !traj) { nyx_set_error("null ctx / traj"); return NYX_HIP_RC_BAD_ARG; }
    return propagate_device(ctx, in, duration_ns, out, stats, traj, hip_stream);
}

// Device views of a staged host batch: `din` lives in ctx->in, `dout` / `dst` in ctx->out.
struct Staged {
    nyx_hip_states_t din, dout;
    nyx_hip_step_stats_t dst;
    bool stm = false;
};

// H2D of a host batch through the pinned mirror (one copy for the SoA block, one for the STMs).
// `upload_stm` false leaves ctx->in.stm allocated but unwritten (covariance mapping starts from identity); true: check_run has seen in->stm.
static int stage_batch(nyx_hip_ctx *ctx, const nyx_hip_states_t *in, Staged &sg, bool upload_stm) {
    const int64_t n = in->n;
    if (int rc = ensure_arrays(ctx, ctx->in, n, false)) return rc;
    if (int rc = ensure_arrays(ctx, ctx->out, n, true)) return rc;
    DevArrays &di = ctx->in, &dq = ctx->out;
    nyx_hip_states_t &din = sg.din;  // (rows the caller left null stay null)
    std::memset(&din, 0, sizeof din);
    din.n = n; din.epoch_ns = di.epoch;
    std::memcpy(di.host(di.epoch), in->epoch_ns, n * sizeof(int64_t));
    for (int k = 0; k < kStateRows; ++k)
        if (const double *h = in->*kStateRow[k].s) std::memcpy(di.host(din.*kStateRow[k].s = di.f[k]), h, n * sizeof(double));
    if (in->step_ns) std::memcpy(di.host(din.step_ns = di.step), in->step_ns, n * sizeof(int64_t));
    HIP_TRY(hipMemcpy(di.dev.p, di.mirror.p, di.state_bytes, hipMemcpyHostToDevice));
    sg.stm = (ctx->host_cfg.flags & NYX_HIP_FLAG_STM) != 0;
    if (sg.stm) {
        for (DevArrays *d : {&di, &dq})
            if (int rc = ensure_stm(ctx, *d, n)) return rc;
        if (upload_stm) HIP_TRY(hipMemcpy(di.stm(), in->stm, (size_t)n * 81 * sizeof(double), hipMemcpyHostToDevice));
    }
    din.stm = sg.stm ? di.stm() : nullptr;
    views_of(dq, n, sg.stm, sg.dout, sg.dst);
    return NYX_HIP_RC_OK;
}

// D2H of ctx->out (states + stats) through the pinned mirror, unpacked into the caller's arrays.
static int fetch_batch(nyx_hip_ctx *ctx, int64_t n, bool stm, nyx_hip_states_t *out, nyx_hip_step_stats_t *stats) {
    DevArrays &dq = ctx->out;
    HIP_TRY(hipMemcpy(dq.mirror.p, dq.dev.p, dq.bytes, hipMemcpyDeviceToHost));
    auto get = [&](auto *h, auto *dev) { if (h) std::memcpy(h, dq.host(dev), n * sizeof *h); };
    get(out->epoch_ns, dq.epoch);
    for (int k = 0; k < kStateRows; ++k) get(out->*kStateRow[k].s, dq.f[k]);
    get(out->step_ns, dq.step);
    if (stm && out->stm) HIP_TRY(hipMemcpy(out->stm, dq.stm(), (size_t)n * 81 * sizeof(double), hipMemcpyDeviceToHost));
    if (stats) {
        get(stats->status, dq.status); get(stats->last_step_ns, dq.last_step); get(stats->last_error, dq.last_error);
        get(stats->last_attempts, dq.last_attempts); get(stats->n_accepted, dq.n_acc); get(stats->n_rejected, dq.n_rej); get(stats->n_evals, dq.n_evals);
    }
    return NYX_HIP_RC_OK;
}

// A nyx_hip_traj_t whose arrays are one device allocation (RAII), laid out by traj_in_block (batch_bind.h).
struct DevTraj {
    nyx_hip_traj_t t;
    DevBuf block;
    size_t slots = 0;
    int64_t n = 0;
    int alloc(int64_t capacity, int64_t n_) {
        n = n_;
        slots = (size_t)capacity * (size_t)n;
        if (int rc = dev_alloc(block, traj_block_bytes(capacity, n))) return rc;
        t = traj_in_block(block.p, capacity, n);
        return NYX_HIP_RC_OK;
    }
    int upload(const nyx_hip_traj_t *h) const { return copy(*h, t, hipMemcpyHostToDevice); }
    int download(nyx_hip_traj_t *h) const { return copy(t, *h, hipMemcpyDeviceToHost); }
    int copy(const nyx_hip_traj_t &from, const nyx_hip_traj_t &to, hipMemcpyKind kind) const {
        HIP_TRY(hipMemcpy(to.len, from.len, (size_t)n * sizeof(int32_t), kind));
        if (!slots) return NYX_HIP_RC_OK;
        HIP_TRY(hipMemcpy(to.epoch_ns, from.epoch_ns, slots * sizeof(int64_t), kind));
        for (int c = 0; c < kCartRows; ++c) HIP_TRY(hipMemcpy(to.*kTrajRow[c], from.*kTrajRow[c], slots * sizeof(double), kind));
        return NYX_HIP_RC_OK;
    }
};

// The one or two trajectory batches of a report staged on the device (`ref`: the second batch - RIC's nominal, a link's
// transmitter - or null: `second` stays empty).
static int stage_trajs(DevTraj &src, DevTraj &second, const nyx_hip_traj_t *traj, int64_t n, const nyx_hip_traj_t *ref, int64_t n_ref) {
    if (int rc = src.alloc(traj->capacity, n)) return rc;
    if (int rc = src.upload(traj)) return rc;
    if (!ref) return NYX_HIP_RC_OK;
    if (int rc = second.alloc(ref->capacity, n_ref)) return rc;
    return second.upload(ref);
}

// The host bracket of a host flavour whose device arrays are one block (dev_block.h): under the context's lock the block `b`
// allocated, the parts `up` copied from their host arrays, `entry(base)` - the device flavour on the block at `base` -, awaited
// (a failure: "`what` failed") and, `timed`, its kernel time read, the parts `down` copied to their host arrays.  A part of size 0 or
// with a null host array is skipped.  `timed` false: the targeter, whose timed launches are the propagator's.
struct HostPart { Part part; const void *host; };
template <int N, typename Entry>
static int host_block(nyx_hip_ctx *ctx, const Block<N> &b, const std::vector<HostPart> &up, const std::vector<HostPart> &down, const char *what, bool timed, Entry entry) {
    CTX_LOCK(ctx);
    HIP_TRY(hipSetDevice(ctx->device));
    DevBuf blk;
    if (int rc = dev_alloc(blk, b.total)) return rc;
    char *base = blk.as<char>();
    for (const HostPart &h : up)
        if (h.part.bytes && h.host) HIP_TRY(hipMemcpy(base + h.part.at, h.host, h.part.bytes, hipMemcpyHostToDevice));
    if (int rc = entry(base)) return rc;
    if (hipDeviceSynchronize() != hipSuccess) { nyx_set_error("%s failed", what); return NYX_HIP_RC_HIP_ERROR; }
    if (timed) read_kernel_ms(ctx);
    for (const HostPart &h : down)
        if (h.part.bytes && h.host) HIP_TRY(hipMemcpy(const_cast<void *>(h.host), base + h.part.at, h.part.bytes, hipMemcpyDeviceToHost));
    return NYX_HIP_RC_OK;
}

// The host bracket of a run: what every such entry checks (check_run, run_host.h; an empty batch is done), the batch staged in the
// context's blocks, `enqueue(sg)` - the entry's launches on the staged views -, awaited and timed, the states and stats fetched, then
// `collect()` - the entry's own copies back.  `upload_stm` false: predict_until.  `traced`: host_propagate (debug_flags 0x400: stderr).
template <typename Enqueue, typename Collect>
static int host_run(nyx_hip_ctx *ctx, const nyx_hip_states_t *in, nyx_hip_states_t *out, nyx_hip_step_stats_t *stats, bool upload_stm, bool traced, Enqueue enqueue, Collect collect) {
    if (Refusal r = check_run(ctx, in, out, upload_stm && ctx && (ctx->host_cfg.flags & NYX_HIP_FLAG_STM))) return refused(r);
    const int64_t n = in->n;
    if (n == 0) return NYX_HIP_RC_OK;
    CTX_LOCK(ctx);
    HIP_TRY(hipSetDevice(ctx->device));
    const bool trace = traced && (ctx->tune.debug_flags & 0x400) != 0;
    if (trace) std::fprintf(stderr, "[nyx_hip] host_propagate n=%lld: staging\n", (long long)n);
    Staged sg;
    if (int rc = stage_batch(ctx, in, sg, upload_stm)) return rc;
    if (trace) std::fprintf(stderr, "[nyx_hip] staged, launching\n");
    if (int rc = enqueue(sg)) return rc;
    if (trace) std::fprintf(stderr, "[nyx_hip] launched (%d helpers, %d waves), synchronising\n", ctx->last_coop_helpers, ctx->host_cfg.n_waves);
    HIP_TRY(hipDeviceSynchronize());
    if (trace) std::fprintf(stderr, "[nyx_hip] kernel done\n");
    read_kernel_ms(ctx);
    if (int rc = fetch_batch(ctx, n, sg.stm, out, stats)) return rc;
    return collect();
}

static int host_propagate(nyx_hip_ctx *ctx, const nyx_hip_states_t *in, int64_t duration_ns, int64_t end_epoch_ns, bool use_end,
                          nyx_hip_states_t *out, nyx_hip_step_stats_t *stats, nyx_hip_traj_t *traj = nullptr) {
    const bool dense = traj && traj->capacity > 0;
    DevTraj dtraj;
    return host_run(ctx, in, out, stats, true, true, [&](Staged &sg) -> int {
        if (int rc = dense ? dtraj.alloc(traj->capacity, in->n) : NYX_HIP_RC_OK) return rc;
        LaunchReq r;
        r.in = &sg.din; r.out = &sg.dout; r.stats = &sg.dst; r.timed = true; r.duration_ns = duration_ns; r.end_epoch_ns = end_epoch_ns; r.use_end = use_end; r.traj = dense ? &dtraj.t : nullptr;
        return launch(ctx, r);
    }, [&]() -> int { return dense ? dtraj.download(traj) : NYX_HIP_RC_OK; });
}

extern "C" int32_t nyx_hip_propagate_batch(nyx_hip_ctx *ctx, const nyx_hip_states_t *in, int64_t duration_ns,
                                           nyx_hip_states_t *out, nyx_hip_step_stats_t *stats) {
    return host_propagate(ctx, in, duration_ns, 0, false, out, stats);
}

extern "C" int32_t nyx_hip_propagate_batch_with_traj(nyx_hip_ctx *ctx, const nyx_hip_states_t *in, int64_t duration_ns,
                                                     nyx_hip_states_t *out, nyx_hip_step_stats_t *stats, nyx_hip_traj_t *traj) {
    if (Refusal r = check_traj_wanted(traj)) return refused(r);
    return host_propagate(ctx, in, duration_ns, 0, false, out, stats, traj);
}

extern "C" int32_t nyx_hip_propagate_until_epoch(nyx_hip_ctx *ctx, const nyx_hip_states_t *in, int64_t end_epoch_ns,
                                                 nyx_hip_states_t *out, nyx_hip_step_stats_t *stats) {
    return host_propagate(ctx, in, 0, end_epoch_ns, true, out, stats);
}

// ---------------------------------------------------------------------------------------------
// One batch over several contexts = several devices of one node, from ONE process (what replaces the rayon par_iter of
// mc/montecarlo.rs:233-253 when the host is not sharded by rank): contiguous index shards (shard_begin, batch_bind.h), one host
// thread per context so that the staging copies and the kernels of the devices overlap, results written in place at the shard's
// offset - the "gather" is free because the arrays are structure-of-arrays.  With a trajectory the shards record into private
// buffers (the step-major layout has the batch size as its stride) and are scattered afterwards.  Trajectories are independent:
// no device-to-device traffic at all.
// ---------------------------------------------------------------------------------------------
extern "C" int32_t nyx_hip_propagate_batch_sharded(nyx_hip_ctx *const *ctxs, int32_t n_ctx, const nyx_hip_states_t *in, int64_t duration_ns,
                                                   nyx_hip_states_t *out, nyx_hip_step_stats_t *stats, nyx_hip_traj_t *traj) {
    if (Refusal r = check_sharded(ctxs, n_ctx, in, out, traj)) return refused(r);
    const int64_t n = in->n, cap = traj ? traj->capacity : 0;
    std::vector<int32_t> rcs((size_t)n_ctx, NYX_HIP_RC_OK);
    std::vector<std::string> errs((size_t)n_ctx);
    std::vector<std::vector<double>> blocks((size_t)n_ctx);  // the shards' trajectory blocks (traj_in_block)
    std::vector<std::thread> threads;
    for (int32_t k = 0; k < n_ctx; ++k) {
        const int64_t lo = shard_begin(n, k, n_ctx), hi = shard_begin(n, k + 1, n_ctx);
        if (hi == lo) continue;
        threads.emplace_back([&, k, lo, hi]() {
            const nyx_hip_states_t vi = states_at(*in, lo, hi - lo);
            nyx_hip_states_t vo = states_at(*out, lo, hi - lo);
            nyx_hip_step_stats_t vs{};
            if (stats) vs = stats_at(*stats, lo);
            int32_t rc;
            if (traj) {
                std::vector<double> &b = blocks[(size_t)k];
                b.assign((traj_block_bytes(cap, hi - lo) + sizeof(double) - 1) / sizeof(double), 0.0);
                nyx_hip_traj_t vt = traj_in_block(b.data(), cap, hi - lo);
                rc = nyx_hip_propagate_batch_with_traj(ctxs[k], &vi, duration_ns, &vo, stats ? &vs : nullptr, &vt);
            } else {
                rc = nyx_hip_propagate_batch(ctxs[k], &vi, duration_ns, &vo, stats ? &vs : nullptr);
            }
            rcs[(size_t)k] = rc;
            if (rc != NYX_HIP_RC_OK) errs[(size_t)k] = nyx_hip_last_error();  // (the message is thread-local)
        });
    }
    for (auto &t : threads) t.join();
    for (int32_t k = 0; k < n_ctx; ++k)
        if (rcs[(size_t)k] != NYX_HIP_RC_OK) { nyx_set_error("shard %d: %s", k, errs[(size_t)k].c_str()); return rcs[(size_t)k]; }
    if (traj)  // the shards' step-major blocks (stride = shard size) into the batch's (stride = n)
        for (int32_t k = 0; k < n_ctx; ++k) {
            const int64_t lo = shard_begin(n, k, n_ctx), m = shard_begin(n, k + 1, n_ctx) - lo;
            if (m) scatter_traj(traj_in_block(blocks[(size_t)k].data(), cap, m), lo, m, *traj, n);
        }
    return NYX_HIP_RC_OK;
}

// ---------------------------------------------------------------------------------------------
// Traj evaluation (md/trajectory/traj.rs:82-162): traj_kernel.hip
// ---------------------------------------------------------------------------------------------
// One timed launch of a context on `stream`, the caller holding its lock: behind the context's previous launch (ev_done), between
// ev0 and ev1 (nyx_hip_last_kernel_ms).  `launch` enqueues the work and returns a hipError_t.
template <typename Launch> static int timed_launch(nyx_hip_ctx *ctx, hipStream_t stream, Launch launch) {
    HIP_TRY(hipSetDevice(ctx->device));
    if (ctx->launched) HIP_TRY(hipStreamWaitEvent(stream, ctx->ev_done, 0));
    HIP_TRY(hipEventRecord(ctx->ev0, stream));
    HIP_TRY(launch());
    HIP_TRY(hipEventRecord(ctx->ev1, stream));
    HIP_TRY(hipEventRecord(ctx->ev_done, stream));
    ctx->launched = true;
    return NYX_HIP_RC_OK;
}

static int traj_eval_device(nyx_hip_ctx *ctx, const nyx_hip_traj_t *traj, int64_t n, const int64_t *query, int64_t m,
                            int64_t step_ns, nyx_hip_traj_t *out, int32_t *status, int mode, hipStream_t stream) {
    if (Refusal r = check_traj_eval(ctx, traj, n, query, m, step_ns, out, status, mode)) return refused(r);
    if (n == 0) return NYX_HIP_RC_OK;
    CTX_LOCK(ctx);
    TrajEvalArgs a;
    std::memset(&a, 0, sizeof a);
    a.src = *traj; a.dst = *out; a.n = n; a.query = query; a.m = m; a.step_ns = step_ns; a.status = status; a.mode = mode;
    return timed_launch(ctx, stream, [&] { return nyx_launch_traj_eval(&a, stream); });
}

extern "C" int32_t nyx_hip_traj_at_device(nyx_hip_ctx *ctx, const nyx_hip_traj_t *traj, int64_t n, const int64_t *query_epoch_ns,
                                          int64_t m, nyx_hip_traj_t *out, int32_t *status, void *hip_stream) {
    return traj_eval_device(ctx, traj, n, query_epoch_ns, m, 0, out, status, TRAJ_MODE_AT, (hipStream_t)hip_stream);
}

extern "C" int32_t nyx_hip_traj_every_device(nyx_hip_ctx *ctx, const nyx_hip_traj_t *traj, int64_t n, int64_t step_ns,
                                             nyx_hip_traj_t *out, void *hip_stream) {
    return traj_eval_device(ctx, traj, n, nullptr, 0, step_ns, out, nullptr, TRAJ_MODE_EVERY, (hipStream_t)hip_stream);
}

// ---------------------------------------------------------------------------------------------
// Ensemble moments of the final states (mc/results.rs:60-245 consumers): moments_kernel.hip
// ---------------------------------------------------------------------------------------------
static int moments_device(nyx_hip_ctx *ctx, const nyx_hip_states_t *s, const int32_t *status, const double *x0, double *out55, hipStream_t stream) {
    if (Refusal r = check_moments(ctx, s, out55, false)) return refused(r);
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(grow(ctx, ctx->d_mom, (MOM_BLOCKS + 1) * MOM_N, cap_exact, PerElement{sizeof(double)}));
    MomArgs a;
    std::memset(&a, 0, sizeof a);
    a.n = s->n;
    for (int k = 0; k < kMomentRows; ++k) { a.f[k] = s->*kStateRow[k].s; a.x0[k] = x0 ? x0[k] : 0.0; }
    a.status = status;
    a.partial = ctx->d_mom.as<double>();
    if (ctx->launched) HIP_TRY(hipStreamWaitEvent(stream, ctx->ev_done, 0));  // (the scratch is the context's: one reduction at a time)
    HIP_TRY(nyx_launch_moments(a, out55, stream));
    HIP_TRY(hipEventRecord(ctx->ev_done, stream));
    ctx->launched = true;
    return NYX_HIP_RC_OK;
}

extern "C" int32_t nyx_hip_ensemble_moments_device(nyx_hip_ctx *ctx, const nyx_hip_states_t *states, const int32_t *status, const double *x0,
                                                   double *out55, void *hip_stream) {
    if (!ctx) { nyx_set_error("null ctx"); return NYX_HIP_RC_BAD_ARG; }
    CTX_LOCK(ctx);
    return moments_device(ctx, states, status, x0, out55, (hipStream_t)hip_stream);
}

// Host arrays: one device block (moments_block), copied row by row; the reduction itself is two small launches into the tail of the context's scratch.
extern "C" int32_t nyx_hip_ensemble_moments(nyx_hip_ctx *ctx, const nyx_hip_states_t *states, const int32_t *status, const double *x0, double *out55) {
    if (Refusal r = check_moments(ctx, states, out55, true)) return refused(r);
    CTX_LOCK(ctx);
    HIP_TRY(hipSetDevice(ctx->device));
    const auto b = moments_block(states->n, status != nullptr);
    DevBuf blk;
    if (int rc = dev_alloc(blk, b.total)) return rc;
    nyx_hip_states_t d{}; d.n = states->n;  // (the staged rows: a device pointer where the caller gave a row)
    for (int k = 0; k < kMomentRows; ++k)
        if (const double *h = states->*kStateRow[k].s) {
            d.*kStateRow[k].s = (double *)(blk.as<char>() + b[k].at);
            if (b[k].bytes) HIP_TRY(hipMemcpy(d.*kStateRow[k].s, h, b[k].bytes, hipMemcpyHostToDevice));
        }
    int32_t *dst = status ? (int32_t *)(blk.as<char>() + b[M_STATUS].at) : nullptr;
    if (b[M_STATUS].bytes) HIP_TRY(hipMemcpy(dst, status, b[M_STATUS].bytes, hipMemcpyHostToDevice));
    HIP_TRY(grow(ctx, ctx->d_mom, (MOM_BLOCKS + 1) * MOM_N, cap_exact, PerElement{sizeof(double)}));
    double *result = ctx->d_mom.as<double>() + (size_t)MOM_BLOCKS * MOM_N;
    if (int rc = moments_device(ctx, &d, dst, x0, result, nullptr)) return rc;
    HIP_TRY(hipMemcpy(out55, result, MOM_N * sizeof(double), hipMemcpyDeviceToHost));
    return NYX_HIP_RC_OK;
}

static int traj_eval_host(nyx_hip_ctx *ctx, const nyx_hip_traj_t *traj, int64_t n, const int64_t *query, int64_t m, int64_t step_ns, nyx_hip_traj_t *out, int32_t *status, int mode) {
    if (Refusal r = check_traj_eval_host(ctx, traj, n, query, m, step_ns, out, status, mode)) return refused(r);
    if (n == 0) return NYX_HIP_RC_OK;
    CTX_LOCK(ctx);
    HIP_TRY(hipSetDevice(ctx->device));
    DevTraj src, dst;
    if (int rc = src.alloc(traj->capacity, n)) return rc;
    if (int rc = dst.alloc(out->capacity, n)) return rc;
    if (int rc = src.upload(traj)) return rc;
    DevBuf d_query, d_status;  // traj_at with m > 0 only: the query epochs [m], the statuses [m][n]
    const size_t qbytes = mode == TRAJ_MODE_AT ? (size_t)m * sizeof(int64_t) : 0, sbytes = mode == TRAJ_MODE_AT ? (size_t)m * (size_t)n * sizeof(int32_t) : 0;
    if (qbytes) {
        if (int rc = dev_alloc(d_query, qbytes)) return rc;
        if (int rc = dev_alloc(d_status, sbytes)) return rc;
        HIP_TRY(hipMemcpy(d_query.p, query, qbytes, hipMemcpyHostToDevice));
    }
    if (int rc = traj_eval_device(ctx, &src.t, n, d_query.as<int64_t>(), m, step_ns, &dst.t, d_status.as<int32_t>(), mode, nullptr)) return rc;
    HIP_TRY(hipDeviceSynchronize());
    read_kernel_ms(ctx);
    if (int rc = dst.download(out)) return rc;
    if (sbytes) HIP_TRY(hipMemcpy(status, d_status.p, sbytes, hipMemcpyDeviceToHost));
    return NYX_HIP_RC_OK;
}

extern "C" int32_t nyx_hip_traj_at(nyx_hip_ctx *ctx, const nyx_hip_traj_t *traj, int64_t n, const int64_t *query_epoch_ns, int64_t m,
                                   nyx_hip_traj_t *out, int32_t *status) {
    return traj_eval_host(ctx, traj, n, query_epoch_ns, m, 0, out, status, TRAJ_MODE_AT);
}

extern "C" int32_t nyx_hip_traj_every(nyx_hip_ctx *ctx, const nyx_hip_traj_t *traj, int64_t n, int64_t step_ns, nyx_hip_traj_t *out) {
    return traj_eval_host(ctx, traj, n, nullptr, 0, step_ns, out, nullptr, TRAJ_MODE_EVERY);
}

// ---------------------------------------------------------------------------------------------
// Fused reports (include/nyx_hip_reports.h): report_kernel.hip
// ---------------------------------------------------------------------------------------------
extern "C" int32_t nyx_hip_reports_sizeof(int32_t which) {
    switch (which) {
    case 0: return (int32_t)sizeof(nyx_hip_values_query_t);
    case 1: return NYX_HIP_REPORTS_VERSION;
    case 2: return NYX_HIP_SP_COUNT;
    case 3: return NYX_HIP_MAX_REPORT_PARAMS;
    default: return -1;
    }
}

// The host flavour of a report: the trajectories (`ref`: RIC's, or null) staged on the device, the outputs one block laid out by
// series_block, `entry(src, ref, outputs)` - the device flavour on those - through host_block, every non-empty part copied back.
// `host.epoch0` / `host.moments` may be null: not asked for.  `what` names the kernel in the message of a failed launch.
struct SeriesOut { double *values; int32_t *len; int64_t *epoch0; double *moments; };
template <typename Entry>
static int series_host(nyx_hip_ctx *ctx, const nyx_hip_traj_t *traj, int64_t n, const nyx_hip_traj_t *ref, int64_t n_ref, int64_t n_params,
                       int64_t capacity, const SeriesOut &host, const char *what, Entry entry) {
    CTX_LOCK(ctx);
    HIP_TRY(hipSetDevice(ctx->device));
    DevTraj src, nominal;
    if (int rc = stage_trajs(src, nominal, traj, n, ref, n_ref)) return rc;
    const auto b = series_block(n_params, capacity, n, host.moments != nullptr, host.epoch0 != nullptr);
    return host_block(ctx, b, {}, {{b[SB_VALUES], host.values}, {b[SB_MOMENTS], host.moments}, {b[SB_EPOCH0], host.epoch0}, {b[SB_LEN], host.len}}, what, true,
                      [&](char *base) {
                          return entry(&src.t, ref ? &nominal.t : nullptr, SeriesOut{part_at<double>(base, b[SB_VALUES]), part_at<int32_t>(base, b[SB_LEN]),
                                                                                      host.epoch0 ? part_at<int64_t>(base, b[SB_EPOCH0]) : nullptr,
                                                                                      host.moments ? part_at<double>(base, b[SB_MOMENTS]) : nullptr});
                      });
}

// What the launch arguments of every report begin with: all zero, then the members the seven have in common (the family's own are
// set behind it).
template <typename Args, typename Query>
static void series_fill(Args &a, const nyx_hip_traj_t *traj, int64_t n, int64_t capacity, double *values, int32_t *len, const Query *q) {
    std::memset(&a, 0, sizeof a);
    a.src = *traj; a.n = n; a.capacity = capacity; a.values = values; a.len = len; a.q = *q;
}

extern "C" int32_t nyx_hip_traj_values_device(nyx_hip_ctx *ctx, const nyx_hip_traj_t *traj, int64_t n, const nyx_hip_values_query_t *q,
                                              int64_t capacity, double *values, int32_t *len, void *hip_stream) {
    if (Refusal r = check_values_series(ctx, traj, n, q, capacity, values, len)) return refused(r);
    if (n == 0) return NYX_HIP_RC_OK;
    hipStream_t stream = (hipStream_t)hip_stream;
    CTX_LOCK(ctx);
    ValuesArgs a;
    series_fill(a, traj, n, capacity, values, len, q);
    if (!(a.q.mu_km3_s2 > 0.0)) a.q.mu_km3_s2 = ctx->host_cfg.mu_central;
    return timed_launch(ctx, stream, [&] { return nyx_launch_traj_values(&a, stream); });
}

extern "C" int32_t nyx_hip_traj_values(nyx_hip_ctx *ctx, const nyx_hip_traj_t *traj, int64_t n, const nyx_hip_values_query_t *q,
                                       int64_t capacity, double *values, int32_t *len) {
    if (Refusal r = check_values_series(ctx, traj, n, q, capacity, values, len)) return refused(r);
    if (n == 0) return NYX_HIP_RC_OK;
    return series_host(ctx, traj, n, nullptr, 0, q->n_params, capacity, {values, len, nullptr, nullptr}, "report kernel",
                       [&](const nyx_hip_traj_t *src, const nyx_hip_traj_t *, const SeriesOut &d) {
                           return nyx_hip_traj_values_device(ctx, src, n, q, capacity, d.values, d.len, nullptr);
                       });
}

// ---------------------------------------------------------------------------------------------
// Ground tracks (include/nyx_hip_groundtrack.h): groundtrack_kernel.hip
// ---------------------------------------------------------------------------------------------
extern "C" int32_t nyx_hip_groundtrack_sizeof(int32_t which) {
    switch (which) {
    case 0: return (int32_t)sizeof(nyx_hip_gt_query_t);
    case 1: return NYX_HIP_GROUNDTRACK_VERSION;
    case 2: return NYX_HIP_GT_COUNT;
    case 3: return NYX_HIP_MAX_GT_PARAMS;
    default: return -1;
    }
}

extern "C" int32_t nyx_hip_traj_ground_track_device(nyx_hip_ctx *ctx, const nyx_hip_traj_t *traj, int64_t n, const nyx_hip_gt_query_t *q,
                                                    int64_t capacity, double *values, int32_t *len, void *hip_stream) {
    if (Refusal r = check_gt_series(ctx, traj, n, q, capacity, values, len)) return refused(r);
    if (n == 0) return NYX_HIP_RC_OK;
    hipStream_t stream = (hipStream_t)hip_stream;
    CTX_LOCK(ctx);
    GroundTrackArgs a;
    series_fill(a, traj, n, capacity, values, len, q);
    return timed_launch(ctx, stream, [&] { return nyx_launch_ground_track(&a, stream); });
}

extern "C" int32_t nyx_hip_traj_ground_track(nyx_hip_ctx *ctx, const nyx_hip_traj_t *traj, int64_t n, const nyx_hip_gt_query_t *q,
                                             int64_t capacity, double *values, int32_t *len) {
    if (Refusal r = check_gt_series(ctx, traj, n, q, capacity, values, len)) return refused(r);
    if (n == 0) return NYX_HIP_RC_OK;
    return series_host(ctx, traj, n, nullptr, 0, q->n_params, capacity, {values, len, nullptr, nullptr}, "ground-track kernel",
                       [&](const nyx_hip_traj_t *src, const nyx_hip_traj_t *, const SeriesOut &d) {
                           return nyx_hip_traj_ground_track_device(ctx, src, n, q, capacity, d.values, d.len, nullptr);
                       });
}

// ---------------------------------------------------------------------------------------------
// Station views (include/nyx_hip_aer.h): aer_kernel.hip
// ---------------------------------------------------------------------------------------------
extern "C" int32_t nyx_hip_aer_sizeof(int32_t which) {
    switch (which) {
    case 0: return (int32_t)sizeof(nyx_hip_aer_query_t);
    case 1: return NYX_HIP_AER_VERSION;
    case 2: return NYX_HIP_AER_COUNT;
    case 3: return NYX_HIP_MAX_AER_PARAMS;
    case 4: return NYX_HIP_MAX_STATIONS;
    default: return -1;
    }
}

extern "C" int32_t nyx_hip_traj_aer_device(nyx_hip_ctx *ctx, const nyx_hip_traj_t *traj, int64_t n, const nyx_hip_aer_query_t *q, int64_t capacity,
                                           double *values, int32_t *len, void *hip_stream) {
    if (Refusal r = check_aer_series(ctx, traj, n, q, capacity, values, len)) return refused(r);
    if (n == 0) return NYX_HIP_RC_OK;
    hipStream_t stream = (hipStream_t)hip_stream;
    CTX_LOCK(ctx);
    AerArgs a;
    series_fill(a, traj, n, capacity, values, len, q);
    return timed_launch(ctx, stream, [&] { return nyx_launch_traj_aer(&a, stream); });
}

extern "C" int32_t nyx_hip_traj_aer(nyx_hip_ctx *ctx, const nyx_hip_traj_t *traj, int64_t n, const nyx_hip_aer_query_t *q, int64_t capacity,
                                    double *values, int32_t *len) {
    if (Refusal r = check_aer_series(ctx, traj, n, q, capacity, values, len)) return refused(r);
    if (n == 0) return NYX_HIP_RC_OK;
    return series_host(ctx, traj, n, nullptr, 0, (int64_t)q->n_stations * q->n_params, capacity, {values, len, nullptr, nullptr}, "station-view kernel",
                       [&](const nyx_hip_traj_t *src, const nyx_hip_traj_t *, const SeriesOut &d) {
                           return nyx_hip_traj_aer_device(ctx, src, n, q, capacity, d.values, d.len, nullptr);
                       });
}

// ---------------------------------------------------------------------------------------------
// Eclipses (include/nyx_hip_eclipse.h): eclipse_kernel.hip
// ---------------------------------------------------------------------------------------------
extern "C" int32_t nyx_hip_ecl_sizeof(int32_t which) {
    switch (which) {
    case 0: return (int32_t)sizeof(nyx_hip_ecl_query_t);
    case 1: return NYX_HIP_ECL_VERSION;
    case 2: return NYX_HIP_ECL_COUNT;
    case 3: return NYX_HIP_MAX_ECL_PARAMS;
    case 4: return NYX_HIP_MAX_ECL_BODIES;
    case 5: return (int32_t)sizeof(nyx_hip_ecl_body_t);
    default: return -1;
    }
}

// check_ecl_series never reads the context (a refusal of the query alone is given for any context pointer); what the query asks of
// the context - its segments, no integration-frame swap - is checked behind it
static Refusal check_ecl(const nyx_hip_ctx *ctx, const nyx_hip_traj_t *traj, int64_t n, const nyx_hip_ecl_query_t *q, int64_t capacity,
                         const double *values, const int32_t *len) {
    if (Refusal r = check_ecl_series(ctx, traj, n, q, capacity, values, len)) return r;
    return check_ecl_context(*q, ctx->host_cfg.n_seg, ctx->swap_n_chain != 0);
}

extern "C" int32_t nyx_hip_traj_eclipse_device(nyx_hip_ctx *ctx, const nyx_hip_traj_t *traj, int64_t n, const nyx_hip_ecl_query_t *q, int64_t capacity,
                                               double *values, int32_t *len, void *hip_stream) {
    if (Refusal r = check_ecl(ctx, traj, n, q, capacity, values, len)) return refused(r);
    if (n == 0) return NYX_HIP_RC_OK;
    hipStream_t stream = (hipStream_t)hip_stream;
    CTX_LOCK(ctx);
    EclArgs a;
    series_fill(a, traj, n, capacity, values, len, q);
    a.records = ctx->d_records.as<double>();
    return timed_launch(ctx, stream, [&] { return nyx_launch_traj_eclipse(&a, ctx->host_cfg.seg, stream); });
}

extern "C" int32_t nyx_hip_traj_eclipse(nyx_hip_ctx *ctx, const nyx_hip_traj_t *traj, int64_t n, const nyx_hip_ecl_query_t *q, int64_t capacity,
                                        double *values, int32_t *len) {
    if (Refusal r = check_ecl(ctx, traj, n, q, capacity, values, len)) return refused(r);
    if (n == 0) return NYX_HIP_RC_OK;
    return series_host(ctx, traj, n, nullptr, 0, q->n_params, capacity, {values, len, nullptr, nullptr}, "eclipse kernel",
                       [&](const nyx_hip_traj_t *src, const nyx_hip_traj_t *, const SeriesOut &d) {
                           return nyx_hip_traj_eclipse_device(ctx, src, n, q, capacity, d.values, d.len, nullptr);
                       });
}

// ---------------------------------------------------------------------------------------------
// Encounter report (include/nyx_hip_frame.h): frame_kernel.hip
// ---------------------------------------------------------------------------------------------
extern "C" int32_t nyx_hip_frame_sizeof(int32_t which) {
    switch (which) {
    case 0: return (int32_t)sizeof(nyx_hip_frame_query_t);
    case 1: return NYX_HIP_FRAME_VERSION;
    case 2: return NYX_HIP_FRM_COUNT;
    case 3: return NYX_HIP_MAX_FRAME_PARAMS;
    default: return -1;
    }
}

// check_frame_series never reads the context; what the query asks of the context - its segments, no integration-frame swap - is
// checked behind it
static Refusal check_frame(const nyx_hip_ctx *ctx, const nyx_hip_traj_t *traj, int64_t n, const nyx_hip_frame_query_t *q, int64_t capacity,
                           const double *values, const int32_t *len) {
    if (Refusal r = check_frame_series(ctx, traj, n, q, capacity, values, len)) return r;
    return check_frame_context(*q, ctx->host_cfg.n_seg, ctx->swap_n_chain != 0);
}

extern "C" int32_t nyx_hip_traj_frame_values_device(nyx_hip_ctx *ctx, const nyx_hip_traj_t *traj, int64_t n, const nyx_hip_frame_query_t *q,
                                                    int64_t capacity, double *values, int32_t *len, void *hip_stream) {
    if (Refusal r = check_frame(ctx, traj, n, q, capacity, values, len)) return refused(r);
    if (n == 0) return NYX_HIP_RC_OK;
    hipStream_t stream = (hipStream_t)hip_stream;
    CTX_LOCK(ctx);
    FrmArgs a;
    series_fill(a, traj, n, capacity, values, len, q);
    a.records = ctx->d_records.as<double>();
    return timed_launch(ctx, stream, [&] { return nyx_launch_traj_frame_values(&a, ctx->host_cfg.seg, stream); });
}

extern "C" int32_t nyx_hip_traj_frame_values(nyx_hip_ctx *ctx, const nyx_hip_traj_t *traj, int64_t n, const nyx_hip_frame_query_t *q,
                                             int64_t capacity, double *values, int32_t *len) {
    if (Refusal r = check_frame(ctx, traj, n, q, capacity, values, len)) return refused(r);
    if (n == 0) return NYX_HIP_RC_OK;
    return series_host(ctx, traj, n, nullptr, 0, q->n_params, capacity, {values, len, nullptr, nullptr}, "encounter kernel",
                       [&](const nyx_hip_traj_t *src, const nyx_hip_traj_t *, const SeriesOut &d) {
                           return nyx_hip_traj_frame_values_device(ctx, src, n, q, capacity, d.values, d.len, nullptr);
                       });
}

// ---------------------------------------------------------------------------------------------
// Lambert transfers (include/nyx_hip_lambert.h): lambert_kernel.hip
// ---------------------------------------------------------------------------------------------
extern "C" int32_t nyx_hip_lambert_sizeof(int32_t which) {
    switch (which) {
    case 0: return (int32_t)sizeof(nyx_hip_lambert_query_t);
    case 1: return NYX_HIP_LAMBERT_VERSION;
    case 2: return NYX_HIP_LMB_COUNT;
    case 3: return NYX_HIP_MAX_LAMBERT_PARAMS;
    case 4: return (int32_t)sizeof(nyx_hip_lambert_grid_query_t);
    case 5: return (int32_t)sizeof(nyx_hip_lambert_chain_t);
    default: return -1;
    }
}

extern "C" int32_t nyx_hip_lambert_batch_device(nyx_hip_ctx *ctx, const double *rv1, const double *rv2, const double *tof_s, int64_t n, double mu_km3_s2,
                                                const nyx_hip_lambert_query_t *q, double *values, int32_t *status, void *hip_stream) {
    if (Refusal r = check_lambert_batch(ctx, rv1, rv2, tof_s, n, mu_km3_s2, q, values, status)) return refused(r);
    if (n == 0) return NYX_HIP_RC_OK;
    hipStream_t stream = (hipStream_t)hip_stream;
    CTX_LOCK(ctx);
    LmbBatchArgs a;
    std::memset(&a, 0, sizeof a);
    a.rv1 = rv1; a.rv2 = rv2; a.tof_s = tof_s; a.n = n; a.mu = mu_km3_s2; a.q = *q; a.values = values; a.status = status;
    return timed_launch(ctx, stream, [&] { return nyx_launch_lambert_batch(&a, stream); });
}

extern "C" int32_t nyx_hip_lambert_batch(nyx_hip_ctx *ctx, const double *rv1, const double *rv2, const double *tof_s, int64_t n, double mu_km3_s2,
                                         const nyx_hip_lambert_query_t *q, double *values, int32_t *status) {
    if (Refusal r = check_lambert_batch(ctx, rv1, rv2, tof_s, n, mu_km3_s2, q, values, status)) return refused(r);
    if (n == 0) return NYX_HIP_RC_OK;
    const auto b = lambert_batch_block(n, q->n_params);
    return host_block(ctx, b, {{b[LBB_RV1], rv1}, {b[LBB_RV2], rv2}, {b[LBB_TOF], tof_s}}, {{b[LBB_VALUES], values}, {b[LBB_STATUS], status}}, "lambert batch kernel", true,
                      [&](char *base) {
                          return nyx_hip_lambert_batch_device(ctx, part_at<double>(base, b[LBB_RV1]), part_at<double>(base, b[LBB_RV2]), part_at<double>(base, b[LBB_TOF]), n,
                                                              mu_km3_s2, q, part_at<double>(base, b[LBB_VALUES]), part_at<int32_t>(base, b[LBB_STATUS]), nullptr);
                      });
}

// check_lambert_grid never reads the context; what the query asks of the context - its segments, no integration-frame swap - is
// checked behind it
static Refusal check_lambert(const nyx_hip_ctx *ctx, const nyx_hip_lambert_grid_query_t *q, const double *values, const int32_t *status) {
    if (Refusal r = check_lambert_grid(ctx, q, values, status)) return r;
    return check_lambert_context(*q, ctx->host_cfg.n_seg, ctx->swap_n_chain != 0);
}

extern "C" int32_t nyx_hip_lambert_grid_device(nyx_hip_ctx *ctx, const nyx_hip_lambert_grid_query_t *q, double *values, int32_t *status, void *hip_stream) {
    if (Refusal r = check_lambert(ctx, q, values, status)) return refused(r);
    if (q->n_dep == 0 || q->n_arr == 0) return NYX_HIP_RC_OK;
    hipStream_t stream = (hipStream_t)hip_stream;
    CTX_LOCK(ctx);
    LmbGridArgs a;
    std::memset(&a, 0, sizeof a);
    a.q = *q; a.records = ctx->d_records.as<double>(); a.values = values; a.status = status;
    return timed_launch(ctx, stream, [&] { return nyx_launch_lambert_grid(&a, ctx->host_cfg.seg, stream); });
}

extern "C" int32_t nyx_hip_lambert_grid(nyx_hip_ctx *ctx, const nyx_hip_lambert_grid_query_t *q, double *values, int32_t *status) {
    if (Refusal r = check_lambert(ctx, q, values, status)) return refused(r);
    if (q->n_dep == 0 || q->n_arr == 0) return NYX_HIP_RC_OK;
    const auto b = lambert_grid_block(q->n_dep, q->n_arr, q->solve.n_params);
    return host_block(ctx, b, {}, {{b[LGB_VALUES], values}, {b[LGB_STATUS], status}}, "lambert grid kernel", true, [&](char *base) {
        return nyx_hip_lambert_grid_device(ctx, q, part_at<double>(base, b[LGB_VALUES]), part_at<int32_t>(base, b[LGB_STATUS]), nullptr);
    });
}

// ---------------------------------------------------------------------------------------------
// The targeter (include/nyx_hip_target.h): target_kernel.hip around the propagator's own launches
// ---------------------------------------------------------------------------------------------
extern "C" int32_t nyx_hip_target_sizeof(int32_t which) {
    switch (which) {
    case 0: return (int32_t)sizeof(nyx_hip_target_query_t);
    case 1: return NYX_HIP_TARGET_VERSION;
    case 2: return NYX_HIP_TGT_STATUS_COUNT;
    case 3: return NYX_HIP_MAX_TARGET_VARS;
    case 4: return (int32_t)sizeof(nyx_hip_target_result_t);
    case 5: return NYX_HIP_MAX_TARGET_OBJS;
    default: return -1;
    }
}

// check_target never reads the context; what the query asks of the context is checked behind it
static Refusal check_tgt(const nyx_hip_ctx *ctx, const nyx_hip_states_t *in, const nyx_hip_target_query_t *q, const nyx_hip_target_result_t *res) {
    if (Refusal r = check_target(ctx, in, q, res)) return r;
    return check_target_context(*q, ctx->host_cfg.n_seg, (ctx->host_cfg.flags & NYX_HIP_FLAG_STM) != 0, ctx->swap_n_chain != 0);
}

// The loop on device arrays: one launch to the correction epoch, the seed, then per round one in-place propagation of the work block,
// the step kernel and the 4-byte read of the runs still active.  Under the context's lock for its whole length.
extern "C" int32_t nyx_hip_target_batch_device(nyx_hip_ctx *ctx, const nyx_hip_states_t *in, const nyx_hip_target_query_t *q, nyx_hip_target_result_t *res,
                                               void *hip_stream) {
    if (Refusal r = check_tgt(ctx, in, q, res)) return refused(r);
    const int64_t n = in->n;
    res->iterations_run = 0;
    if (n == 0) return NYX_HIP_RC_OK;
    hipStream_t stream = (hipStream_t)hip_stream;
    CTX_LOCK(ctx);
    HIP_TRY(hipSetDevice(ctx->device));
    if (ctx->launched) HIP_TRY(hipEventSynchronize(ctx->ev_done));  // (the blocks below may grow: nothing of this context is in flight then)
    const int64_t rows = (int64_t)(1 + q->n_vars) * n;
    if (int rc = ensure_arrays(ctx, ctx->out, n, true)) return rc;
    if (int rc = ensure_arrays(ctx, ctx->work, rows, true)) return rc;
    // what the runs keep between the rounds, their flags and the counters: one block of the context
    HIP_TRY(grow(ctx, ctx->d_tgt, n, cap_batch, [](int64_t cap) { return target_keep_block(cap).total; }, /*zero=*/true));
    const auto keep = target_keep_block(ctx->d_tgt.cap);
    nyx_hip_states_t xs, ws;
    nyx_hip_step_stats_t xss, wss;
    views_of(ctx->out, n, false, xs, xss);
    views_of(ctx->work, rows, false, ws, wss);
    ws.step_ns = nullptr;  // (every round starts from the context's initial step, as a fresh batch does)
    LaunchReq leg;
    leg.in = in; leg.out = &xs; leg.stats = &xss; leg.use_end = true; leg.end_epoch_ns = q->correction_epoch_ns; leg.stream = hip_stream;
    if (int rc = launch(ctx, leg)) return rc;
    TgtArgs a;
    std::memset(&a, 0, sizeof a);
    a.q = *q; a.n = n; a.cap = ctx->d_tgt.cap;
    a.start = tgt_rows(xs, xss.status);
    a.work = tgt_rows(ws, wss.status);
    a.keep = part_at<double>(ctx->d_tgt.as<char>(), keep[TK_KEEP]);
    a.flag = part_at<int32_t>(ctx->d_tgt.as<char>(), keep[TK_FLAG]);
    a.active = part_at<int32_t>(ctx->d_tgt.as<char>(), keep[TK_ACTIVE]);
    a.chain = resolve_chain(chain_view(*q), ctx->host_cfg.seg);
    a.records = ctx->d_records.as<double>();
    a.o_status = res->status; a.o_iterations = res->iterations; a.o_correction = res->correction; a.o_errors = res->achieved_errors;
    a.corrected = tgt_rows(res->corrected, nullptr);
    a.achieved = tgt_rows(res->achieved, nullptr);
    HIP_TRY(hipMemsetAsync(a.active, 0, (size_t)(q->iterations + 2) * sizeof(int32_t), stream));
    HIP_TRY(nyx_launch_target_seed(&a, stream));
    LaunchReq round;
    round.in = &ws; round.out = &ws; round.stats = &wss; round.use_end = true; round.end_epoch_ns = q->achievement_epoch_ns; round.stream = hip_stream;
    int32_t rounds = 0;
    for (int it = 0; it <= q->iterations; ++it) {
        if (int rc = launch(ctx, round)) return rc;
        a.it = it;
        HIP_TRY(nyx_launch_target_step(&a, stream));
        int32_t live = 0;
        HIP_TRY(hipMemcpyAsync(&live, a.active + it, sizeof live, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        rounds = it + 1;
        if (live == 0) break;
    }
    HIP_TRY(hipEventRecord(ctx->ev_done, stream));
    res->iterations_run = rounds;
    return NYX_HIP_RC_OK;
}

extern "C" int32_t nyx_hip_target_batch(nyx_hip_ctx *ctx, const nyx_hip_states_t *in, const nyx_hip_target_query_t *q, nyx_hip_target_result_t *res) {
    if (Refusal r = check_tgt(ctx, in, q, res)) return refused(r);
    const int64_t n = in->n;
    res->iterations_run = 0;
    if (n == 0) return NYX_HIP_RC_OK;
    CTX_LOCK(ctx);
    HIP_TRY(hipSetDevice(ctx->device));
    Staged sg;
    if (int rc = stage_batch(ctx, in, sg, false)) return rc;
    // the outputs: one device block (target_block), every row of it the caller gave an array for copied back
    const auto b = target_block(n, q->n_vars, q->n_objs);
    std::vector<HostPart> down = {{b[TGB_CORRECTION], res->correction}, {b[TGB_ERRORS], res->achieved_errors}, {b[TGB_STATUS], res->status}, {b[TGB_ITERATIONS], res->iterations}};
    const nyx_hip_states_t *host[2] = {&res->corrected, &res->achieved};
    for (int s = 0; s < 2; ++s) {
        down.push_back({target_row(b, TGB_CORRECTED + s, 0), host[s]->epoch_ns});
        for (int k = 0; k < kStateRows; ++k) down.push_back({target_row(b, TGB_CORRECTED + s, 1 + k), host[s]->*kStateRow[k].s});
    }
    nyx_hip_target_result_t d;
    std::memset(&d, 0, sizeof d);
    if (int rc = host_block(ctx, b, {}, down, "targeter kernels", false, [&](char *base) {
            bind_target_result(d, base, b);
            return nyx_hip_target_batch_device(ctx, &sg.din, q, &d, nullptr);
        }))
        return rc;
    res->iterations_run = d.iterations_run;
    return NYX_HIP_RC_OK;
}

// ---------------------------------------------------------------------------------------------
// RIC dispersions (include/nyx_hip_ric.h): ric_kernel.hip
// ---------------------------------------------------------------------------------------------
extern "C" int32_t nyx_hip_ric_sizeof(int32_t which) {
    switch (which) {
    case 0: return (int32_t)sizeof(nyx_hip_ric_query_t);
    case 1: return NYX_HIP_RIC_VERSION;
    case 2: return NYX_HIP_RIC_MOMENTS;
    case 3: return NYX_HIP_RIC_MAX_WINDOW;
    default: return -1;
    }
}

// (n == 0 is launched, unlike the two reports above: the moments of no run are zeros)
extern "C" int32_t nyx_hip_traj_ric_diff_device(nyx_hip_ctx *ctx, const nyx_hip_traj_t *traj, int64_t n, const nyx_hip_traj_t *ref,
                                                int64_t n_ref, const nyx_hip_ric_query_t *q, int64_t capacity, double *values, int32_t *len,
                                                int64_t *epoch0_ns, double *moments, void *hip_stream) {
    if (Refusal r = check_ric_series(ctx, traj, n, ref, n_ref, q, capacity, values, len)) return refused(r);
    hipStream_t stream = (hipStream_t)hip_stream;
    CTX_LOCK(ctx);
    RicArgs a;
    series_fill(a, traj, n, capacity, values, len, q);
    a.ref = *ref; a.n_ref = n_ref; a.epoch0 = epoch0_ns; a.moments = moments;
    return timed_launch(ctx, stream, [&] {
        if (n > 0) return nyx_launch_ric_diff(&a, stream);
        // no run: every sample has count 0
        return moments ? hipMemsetAsync(moments, 0, (size_t)capacity * NYX_HIP_RIC_MOMENTS * sizeof(double), stream) : hipSuccess;
    });
}

extern "C" int32_t nyx_hip_traj_ric_diff(nyx_hip_ctx *ctx, const nyx_hip_traj_t *traj, int64_t n, const nyx_hip_traj_t *ref, int64_t n_ref,
                                         const nyx_hip_ric_query_t *q, int64_t capacity, double *values, int32_t *len, int64_t *epoch0_ns,
                                         double *moments) {
    if (Refusal r = check_ric_series(ctx, traj, n, ref, n_ref, q, capacity, values, len)) return refused(r);
    return series_host(ctx, traj, n, ref, n_ref, 6, capacity, {values, len, epoch0_ns, moments}, "RIC kernel",
                       [&](const nyx_hip_traj_t *src, const nyx_hip_traj_t *nominal, const SeriesOut &d) {
                           return nyx_hip_traj_ric_diff_device(ctx, src, n, nominal, n_ref, q, capacity, d.values, d.len, d.epoch0, d.moments, nullptr);
                       });
}

// ---------------------------------------------------------------------------------------------
// Link report (include/nyx_hip_link.h): link_kernel.hip
// ---------------------------------------------------------------------------------------------
extern "C" int32_t nyx_hip_link_sizeof(int32_t which) {
    switch (which) {
    case 0: return (int32_t)sizeof(nyx_hip_link_query_t);
    case 1: return NYX_HIP_LINK_VERSION;
    case 2: return NYX_HIP_LNK_COUNT;
    case 3: return NYX_HIP_MAX_LINK_PARAMS;
    case 4: return NYX_HIP_MAX_LINK_BODIES;
    default: return -1;
    }
}

// check_link_series never reads the context; what the query asks of the context - its segments, no integration-frame swap - is
// checked behind it
static Refusal check_link(const nyx_hip_ctx *ctx, const nyx_hip_traj_t *traj, int64_t n, const nyx_hip_traj_t *ref, int64_t n_ref,
                          const nyx_hip_link_query_t *q, int64_t capacity, const double *values, const int32_t *len) {
    if (Refusal r = check_link_series(ctx, traj, n, ref, n_ref, q, capacity, values, len)) return r;
    return check_link_context(*q, ctx->host_cfg.n_seg, ctx->swap_n_chain != 0);
}

extern "C" int32_t nyx_hip_traj_link_device(nyx_hip_ctx *ctx, const nyx_hip_traj_t *traj, int64_t n, const nyx_hip_traj_t *ref, int64_t n_ref,
                                            const nyx_hip_link_query_t *q, int64_t capacity, double *values, int32_t *len, int64_t *epoch0_ns,
                                            void *hip_stream) {
    if (Refusal r = check_link(ctx, traj, n, ref, n_ref, q, capacity, values, len)) return refused(r);
    if (n == 0) return NYX_HIP_RC_OK;
    hipStream_t stream = (hipStream_t)hip_stream;
    CTX_LOCK(ctx);
    LnkArgs a;
    series_fill(a, traj, n, capacity, values, len, q);
    a.ref = *ref; a.n_ref = n_ref; a.epoch0 = epoch0_ns; a.records = ctx->d_records.as<double>();
    return timed_launch(ctx, stream, [&] { return nyx_launch_traj_link(&a, ctx->host_cfg.seg, stream); });
}

extern "C" int32_t nyx_hip_traj_link(nyx_hip_ctx *ctx, const nyx_hip_traj_t *traj, int64_t n, const nyx_hip_traj_t *ref, int64_t n_ref,
                                     const nyx_hip_link_query_t *q, int64_t capacity, double *values, int32_t *len, int64_t *epoch0_ns) {
    if (Refusal r = check_link(ctx, traj, n, ref, n_ref, q, capacity, values, len)) return refused(r);
    if (n == 0) return NYX_HIP_RC_OK;
    return series_host(ctx, traj, n, ref, n_ref, q->n_params, capacity, {values, len, epoch0_ns, nullptr}, "link kernel",
                       [&](const nyx_hip_traj_t *src, const nyx_hip_traj_t *tx, const SeriesOut &d) {
                           return nyx_hip_traj_link_device(ctx, src, n, tx, n_ref, q, capacity, d.values, d.len, d.epoch0, nullptr);
                       });
}

// ---------------------------------------------------------------------------------------------
// Ensemble statistics of a report (include/nyx_hip_stats.h): stats_kernel.hip
// ---------------------------------------------------------------------------------------------
extern "C" int32_t nyx_hip_stats_sizeof(int32_t which) {
    switch (which) {
    case 0: return (int32_t)sizeof(nyx_hip_stats_query_t);
    case 1: return NYX_HIP_STATS_VERSION;
    case 2: return NYX_HIP_STAT_FIXED;
    case 3: return NYX_HIP_MAX_STAT_PROBS;
    case 4: return NYX_HIP_SERIES_COUNT;
    default: return -1;
    }
}

// (n == 0 is launched: every (row, sample) gets the empty pattern)
extern "C" int32_t nyx_hip_series_stats_device(nyx_hip_ctx *ctx, const double *values, const int32_t *len, const int32_t *status, int64_t n_rows,
                                               int64_t capacity, int64_t n, const nyx_hip_stats_query_t *q, double *stats, void *hip_stream) {
    if (Refusal r = check_series_stats(ctx, values, len, n_rows, capacity, n, q, stats)) return refused(r);
    hipStream_t stream = (hipStream_t)hip_stream;
    CTX_LOCK(ctx);
    StatArgs a;
    std::memset(&a, 0, sizeof a);
    a.values = values; a.len = len; a.status = status; a.stats = stats; a.capacity = capacity; a.n = (int32_t)n; a.q = *q;
    return timed_launch(ctx, stream, [&] { return nyx_launch_series_stats(&a, n_rows, stream); });
}

extern "C" int32_t nyx_hip_series_stats(nyx_hip_ctx *ctx, const double *values, const int32_t *len, const int32_t *status, int64_t n_rows,
                                        int64_t capacity, int64_t n, const nyx_hip_stats_query_t *q, double *stats) {
    if (Refusal r = check_series_stats(ctx, values, len, n_rows, capacity, n, q, stats)) return refused(r);
    const auto b = stats_block(n_rows, capacity, n, q->n_probs, status != nullptr);
    return host_block(ctx, b, {{b[STB_VALUES], values}, {b[STB_LEN], len}, {b[STB_STATUS], status}}, {{b[STB_STATS], stats}}, "statistics kernel", true, [&](char *base) {
        return nyx_hip_series_stats_device(ctx, part_at<double>(base, b[STB_VALUES]), part_at<int32_t>(base, b[STB_LEN]),
                                           status ? part_at<int32_t>(base, b[STB_STATUS]) : nullptr, n_rows, capacity, n, q, part_at<double>(base, b[STB_STATS]), nullptr);
    });
}

// The seven reports by their kind (nyx_hip_series_kind), stated once for the fused entry below.  `launch` false: the refusals of the
// report itself, by its own check function, and nothing else (`values` / `len`: any non-null pointers, none is read); true: its
// *_device entry - which begins with that check - on the default stream.
static int series_by_kind(bool launch, nyx_hip_ctx *ctx, int32_t kind, const nyx_hip_traj_t *traj, int64_t n, const nyx_hip_traj_t *ref, int64_t n_ref,
                          const void *query, int64_t capacity, double *values, int32_t *len, int64_t *epoch0) {
    auto checked = [](const Refusal &r) { return r ? refused(r) : NYX_HIP_RC_OK; };
    auto one = [&](auto *q, auto check, auto entry) -> int {   // a report of one batch
        return launch ? entry(ctx, traj, n, q, capacity, values, len, nullptr) : checked(check(ctx, traj, n, q, capacity, values, len));
    };
    switch (kind) {
    case NYX_HIP_SERIES_VALUES: return one((const nyx_hip_values_query_t *)query, check_values_series, nyx_hip_traj_values_device);
    case NYX_HIP_SERIES_GROUND_TRACK: return one((const nyx_hip_gt_query_t *)query, check_gt_series, nyx_hip_traj_ground_track_device);
    case NYX_HIP_SERIES_AER: return one((const nyx_hip_aer_query_t *)query, check_aer_series, nyx_hip_traj_aer_device);
    case NYX_HIP_SERIES_ECLIPSE: return one((const nyx_hip_ecl_query_t *)query, check_ecl, nyx_hip_traj_eclipse_device);
    case NYX_HIP_SERIES_FRAME: return one((const nyx_hip_frame_query_t *)query, check_frame, nyx_hip_traj_frame_values_device);
    case NYX_HIP_SERIES_LINK:
        return launch ? nyx_hip_traj_link_device(ctx, traj, n, ref, n_ref, (const nyx_hip_link_query_t *)query, capacity, values, len, epoch0, nullptr)
                      : checked(check_link(ctx, traj, n, ref, n_ref, (const nyx_hip_link_query_t *)query, capacity, values, len));
    default:   // NYX_HIP_SERIES_RIC
        return launch ? nyx_hip_traj_ric_diff_device(ctx, traj, n, ref, n_ref, (const nyx_hip_ric_query_t *)query, capacity, values, len, epoch0, nullptr, nullptr)
                      : checked(check_ric_series(ctx, traj, n, ref, n_ref, (const nyx_hip_ric_query_t *)query, capacity, values, len));
    }
}

// The fused host entry: the trajectories staged as series_host stages them (none where there is no run), the report's device entry
// into the values of a stats_block, the reducer behind it on the same stream; only the statistics, the lengths and - of a report with a
// second batch - the first epochs come back (those from a device array of their own: the block has no part for them).
extern "C" int32_t nyx_hip_traj_series_stats(nyx_hip_ctx *ctx, int32_t kind, const nyx_hip_traj_t *traj, int64_t n, const nyx_hip_traj_t *ref,
                                             int64_t n_ref, const void *query, int64_t query_size, int64_t capacity, const int32_t *status,
                                             const nyx_hip_stats_query_t *sq, double *stats, int32_t *len, int64_t *epoch0_ns) {
    if (Refusal r = check_traj_series_stats(ctx, kind, traj, ref, query, query_size, sq, stats, len)) return refused(r);
    if (int rc = series_by_kind(false, ctx, kind, traj, n, ref, n_ref, query, capacity, stats, len, nullptr)) return rc;
    if (n > INT32_MAX) return refused(bad_arg("traj_series_stats: n must be 0 .. 2^31 - 1"));
    CTX_LOCK(ctx);
    HIP_TRY(hipSetDevice(ctx->device));
    DevTraj src, second;
    if (n > 0)
        if (int rc = stage_trajs(src, second, traj, n, ref, n_ref)) return rc;
    const int64_t rows = series_kind_rows(kind, query);
    const auto b = stats_block(rows, capacity, n, sq->n_probs, status != nullptr);
    DevBuf first;
    const size_t first_bytes = (ref && epoch0_ns) ? (size_t)n * sizeof(int64_t) : 0;
    if (first_bytes)
        if (int rc = dev_alloc(first, first_bytes)) return rc;
    if (int rc = host_block(ctx, b, {{b[STB_STATUS], status}}, {{b[STB_STATS], stats}, {b[STB_LEN], len}}, "report or statistics kernel", true, [&](char *base) -> int {
            double *d_values = part_at<double>(base, b[STB_VALUES]);
            int32_t *d_len = part_at<int32_t>(base, b[STB_LEN]);
            if (n > 0)
                if (int rc = series_by_kind(true, ctx, kind, &src.t, n, ref ? &second.t : nullptr, n_ref, query, capacity, d_values, d_len, first.as<int64_t>())) return rc;
            return nyx_hip_series_stats_device(ctx, d_values, d_len, status ? part_at<int32_t>(base, b[STB_STATUS]) : nullptr, rows, capacity, n, sq,
                                               part_at<double>(base, b[STB_STATS]), nullptr);
        }))
        return rc;
    if (first_bytes) HIP_TRY(hipMemcpy(epoch0_ns, first.p, first_bytes, hipMemcpyDeviceToHost));
    return NYX_HIP_RC_OK;
}

// ---------------------------------------------------------------------------------------------
// Stop conditions (propagators/event.rs:88-211): propagation with the crossing counter, then the root search
// ---------------------------------------------------------------------------------------------
extern "C" int32_t nyx_hip_propagate_until_event(nyx_hip_ctx *ctx, const nyx_hip_states_t *in, int64_t max_duration_ns,
                                                 const nyx_hip_event_t *event, nyx_hip_states_t *out, nyx_hip_step_stats_t *stats,
                                                 nyx_hip_traj_t *traj, int32_t *crossings) {
    if (Refusal r = check_event(ctx, event, traj)) return refused(r);
    DevTraj dtraj;
    DevBuf evbuf, evdesc;  // prev, count, found (event_block); the event descriptor itself
    DevBatch ev{};
    return host_run(ctx, in, out, stats, true, false, [&](Staged &sg) -> int {
        const int64_t n = in->n;
        if (int rc = dtraj.alloc(traj->capacity, n)) return rc;
        const auto b = event_block(n);
        if (int rc = dev_alloc(evbuf, b.total)) return rc;
        if (int rc = dev_alloc(evdesc, sizeof(nyx_hip_event_t))) return rc;
        HIP_TRY(hipMemcpy(evdesc.p, event, sizeof(nyx_hip_event_t), hipMemcpyHostToDevice));
        ev.ev = evdesc.as<nyx_hip_event_t>(); ev.ev_mu = ctx->host_cfg.mu_central;
        char *base = evbuf.as<char>();
        ev.ev_prev = (double *)(base + b[E_PREV].at); ev.ev_count = (int32_t *)(base + b[E_COUNT].at); ev.ev_found = (int32_t *)(base + b[E_FOUND].at);
        HIP_TRY(hipMemset(evbuf.p, 0, b.total));
        LaunchReq r;
        r.in = &sg.din; r.out = &sg.dout; r.stats = &sg.dst; r.duration_ns = max_duration_ns; r.traj = &dtraj.t; r.ev = &ev; r.timed = true;
        if (int rc = launch(ctx, r)) return rc;
        EventSearchArgs a{};
        a.traj = dtraj.t; a.n = n; a.ev = *event; a.mu = ctx->host_cfg.mu_central; a.found = ev.ev_found; a.status = sg.dst.status; a.epoch_ns = sg.dout.epoch_ns;
        for (int c = 0; c < kCartRows; ++c) a.state[c] = sg.dout.*kStateRow[c].s;
        HIP_TRY(nyx_launch_event_search(&a, nullptr));
        return NYX_HIP_RC_OK;
    }, [&]() -> int {
        if (int rc = dtraj.download(traj)) return rc;
        if (crossings) HIP_TRY(hipMemcpy(crossings, ev.ev_count, (size_t)in->n * sizeof(int32_t), hipMemcpyDeviceToHost));
        return NYX_HIP_RC_OK;
    });
}

// ---------------------------------------------------------------------------------------------
// Covariance mapping (od/process/mod.rs:440-486): segment launches + predict_kernel.hip, one stream, no host round trip
// ---------------------------------------------------------------------------------------------

extern "C" int32_t nyx_hip_predict_until(nyx_hip_ctx *ctx, const nyx_hip_states_t *in, const nyx_hip_predict_t *cfg,
                                         nyx_hip_estimates_t *est, nyx_hip_states_t *out, nyx_hip_step_stats_t *stats,
                                         nyx_hip_predict_history_t *hist) {
    if (Refusal r = check_predict(ctx, ctx ? ctx->host_cfg.flags : 0, cfg, est, hist)) return refused(r);
    const nyx_hip_predict_history_t h = hist ? *hist : nyx_hip_predict_history_t{};  // (no history: every array null)
    const nyx_hip_step_stats_t st = stats ? *stats : nyx_hip_step_stats_t{};
    DevBuf block, pa_dev;  // the filter's working memory, one allocation (predict_block); the device copy of a fused loop's arguments
    const auto b = predict_block(in ? in->n : 0, h);  // (used behind check_run only)
    return host_run(ctx, in, out, stats, false, false, [&](Staged &sg) -> int {
        const int64_t n = in->n;
        if (int rc = dev_alloc(block, b.total)) return rc;
        char *base = block.as<char>();
        HIP_TRY(hipMemcpy(base + b[P_COVAR].at, est->covar, b[P_COVAR].bytes, hipMemcpyHostToDevice));
        if (est->state_dev) HIP_TRY(hipMemcpy(base + b[P_SDEV].at, est->state_dev, b[P_SDEV].bytes, hipMemcpyHostToDevice));
        // zeros in the history (a run's unwritten last slots are copied back: zeros, as the oracle leaves them) and, in front of it, in the deviations of a caller who gives none
        const size_t zero = b[est->state_dev ? P_H_EPOCH : P_SDEV].at;
        if (b[P_STATUS].at > zero) HIP_TRY(hipMemsetAsync(base + zero, 0, b[P_STATUS].at - zero, nullptr));
        PredictArgs a{};
        a.n = n; a.cfg = *cfg; a.epoch = sg.dout.epoch_ns;
        for (int k = 0; k < kMomentRows; ++k) a.s9[k] = sg.dout.*kStateRow[k].s;
        a.seg_status = sg.dst.status; a.seg_n_acc = sg.dst.n_accepted; a.seg_n_rej = sg.dst.n_rejected; a.seg_n_evals = sg.dst.n_evals;
        bind_predict(a, base, b);
        a.hist.capacity = h.capacity;
        hipStream_t stream = nullptr;
        HIP_TRY(hipEventRecord(ctx->ev0, stream));
        // segment 0 reads the caller's states (ctx->in) with an identity STM and writes ctx->out; later segments run in place
        a.stm = sg.din.stm;
        HIP_TRY(nyx_launch_predict_init(&a, sg.din.epoch_ns, stream));
        // the segment launches are measured once per context, on the staged states (identity STM set above): see calibrates_first,
        // launch_plan.h (the shape of their launches, planned on a copy of the descriptor: each launch plans for itself)
        const std::unique_ptr<DevCfg> dc(new DevCfg(ctx->host_cfg));
        SchedShape shape = ctx->shape;
        const LaunchPlan p = plan_launch(plan_inputs(ctx), *dc, shape, n, true);
        if (calibrates_first(plan_inputs(ctx), ctx->host_cfg, weight_key(*dc, p.n_waves, p.quad, p.coop.run), p.n_waves, n, /*min_n=*/16, /*plain=*/true, 0, /*min_steps=*/0)) {
            if (int rc = calibrate(ctx, &sg.din, stream)) return rc;
            HIP_TRY(hipEventRecord(ctx->ev0, stream));  // (the timed region is the segment loop, not the one-off calibration)
        }
        a.stm = sg.dout.stm;
        // Round 6: the whole loop in ONE launch - the workgroups stay resident, the integrator wave performs the time updates of its
        // trajectories at every segment boundary (propagate_kernel.hip, segment_update; DevBatch.pred = a device copy of `a`).  A segment
        // launch cost ~30 us beyond its force evaluations (tools/seg_cost.py), a fifth of BASELINE config 4's loop.  The launch-per-segment
        // loop of rounds 2-5 stays for the integration-frame swap (translated in and out per segment, od/process/mod.rs:453-468) and as
        // the A/B reference (debug_flags 0x20000000): same states, STMs and covariances.  Which of the two: predict_fused (launch_plan.h).
        LaunchReq seg;  // (per-trajectory durations; segment 0 reads the staged states, the later ones run in place)
        seg.in = &sg.din; seg.out = &sg.dout; seg.stats = &sg.dst; seg.dur_ns = a.dur; seg.stream = stream;
        if (predict_fused(plan_inputs(ctx), ctx->host_cfg, n, ctx->swap_n_chain)) {
            if (int rc = dev_alloc(pa_dev, sizeof(PredictArgs))) return rc;
            HIP_TRY(hipMemcpyAsync(pa_dev.p, &a, sizeof(PredictArgs), hipMemcpyHostToDevice, stream));
            ctx->fused_pred = (const PredictArgs *)pa_dev.p;
            const int rc = launch(ctx, seg);
            ctx->fused_pred = nullptr;
            if (rc) return rc;
            // the kernel's counters run over the whole loop
            HIP_TRY(hipMemcpyAsync(a.acc_n_acc, sg.dst.n_accepted, (size_t)n * 8, hipMemcpyDeviceToDevice, stream));
            HIP_TRY(hipMemcpyAsync(a.acc_n_rej, sg.dst.n_rejected, (size_t)n * 8, hipMemcpyDeviceToDevice, stream));
            HIP_TRY(hipMemcpyAsync(a.acc_n_evals, sg.dst.n_evals, (size_t)n * 8, hipMemcpyDeviceToDevice, stream));
        } else
        for (int64_t s = predict_segments(in->epoch_ns, n, cfg->end_epoch_ns, cfg->max_step_ns); s > 0; --s) {
            if (int rc = launch(ctx, seg)) return rc;
            HIP_TRY(nyx_launch_time_update(&a, stream));
            seg.in = &sg.dout;
        }
        HIP_TRY(hipEventRecord(ctx->ev1, stream));
        return NYX_HIP_RC_OK;
    }, [&]() -> int {
        // after the fetch of the last segment's stats: the first failing status, the summed counters; every part the caller asked for
        const struct { void *host; int part; } back[] = {
            {est->covar, P_COVAR}, {est->state_dev, P_SDEV}, {st.status, P_STATUS}, {st.n_accepted, P_ACC_N_ACC}, {st.n_rejected, P_ACC_N_REJ}, {st.n_evals, P_ACC_N_EVALS},
            {h.n_updates, P_N_UPDATES}, {h.epoch_ns, P_H_EPOCH}, {h.state, P_H_STATE}, {h.stm, P_H_STM}, {h.covar, P_H_COVAR}, {h.state_dev, P_H_SDEV}};
        for (const auto &c : back)
            if (c.host && b[c.part].bytes) HIP_TRY(hipMemcpy(c.host, block.as<char>() + b[c.part].at, b[c.part].bytes, hipMemcpyDeviceToHost));
        return NYX_HIP_RC_OK;
    });
}

// Introspection for tests / DESIGN.md: rows per wave of the SOLO column schedule an n_waves workgroup of this context would walk.
// loads[16].  Planned on a copy of the descriptor: the context keeps the schedules its last launch uploaded.
extern "C" int32_t nyx_hip_debug_schedule(nyx_hip_ctx *ctx, int32_t n_waves, int32_t *loads /* [16] */) {
    if (!ctx || !loads || n_waves < 1 || n_waves > DEV_MAX_WAVES) return NYX_HIP_RC_BAD_ARG;
    CTX_LOCK(ctx);
    const std::unique_ptr<DevCfg> dc(new DevCfg(ctx->host_cfg));
    build_schedule(plan_inputs(ctx), *dc, ctx->shape, n_waves);
    for (int w = 0; w < DEV_MAX_WAVES; ++w) loads[w] = rows_of(ctx, dc->sched[DEV_SCHED_SOLO], w);
    return NYX_HIP_RC_OK;
}
