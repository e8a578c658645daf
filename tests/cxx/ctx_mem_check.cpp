// Stand-alone check of the memory of a context (nyx_amd/csrc/ctx_mem.h) and of build_run_stream (nyx_amd/csrc/ctx_build.h) - g++
// only, no HIP, no GPU (tests/test_ctx_mem.py).
//   ctx_mem_check JGM3_70x70_F64
// The three blocks against the expressions abi.cpp carried inline in the commit before the header had them, restated here; the
// owner on a counting allocator; build_run_stream against the function as abi.cpp carried it, on the schedules of three fields.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <map>
#include <memory>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "../../nyx_amd/csrc/ctx_build.h"
#include "../../nyx_amd/csrc/ctx_mem.h"
#include "launch_plan_cases.h"

static int g_fail = 0;
#define CHECK(cond, ...)                                                              \
    do {                                                                              \
        if (!(cond)) {                                                                \
            if (++g_fail <= 30) { std::printf("FAIL %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                             \
    } while (0)

#include "block_check.h"

// ---------------------------------------------------------------------------------------------
// the layouts
// ---------------------------------------------------------------------------------------------
static const int64_t kCaps[] = {1, 63, 64, 65, 1023, 1024, 1025, 10000, 1000000};

static void check_roundings() {
    for (int64_t n : kCaps) {
        // the parent's expressions: ensure_arrays / ensure_target_keep, ensure_stm, the textbook history, the swap copy, mailbox_acquire
        CHECK(cap_batch(n) == (std::max<int64_t>(n, 1024) + 63) / 64 * 64, "n=%lld", (long long)n);
        CHECK(cap_stm(n) == std::max<int64_t>(n, 1024), "n=%lld", (long long)n);
        CHECK(cap_stm_hist(n) == (n + 63) / 64 * 64, "n=%lld", (long long)n);
        CHECK(cap_exact(n) == n, "n=%lld", (long long)n);
        CHECK(cap_mailbox(n) == (n + 255) / 256 * 256, "n=%lld", (long long)n);
        for (int64_t c : {cap_batch(n), cap_stm(n), cap_stm_hist(n), cap_exact(n), cap_mailbox(n)}) CHECK(c >= n, "n=%lld", (long long)n);
    }
}

static void check_arrays_block() {
    for (int64_t cap : kCaps)
        for (int stats = 0; stats < 2; ++stats) {
            const auto b = arrays_block(cap, stats != 0);
            // ensure_arrays of the parent: p = dblock; epoch, step, f[0..12] a slot each; with stats five more slots, then two rows of cap * 4
            const size_t slot = (size_t)cap * 8;
            const size_t n64 = 15 + (stats ? 5 : 0);
            const size_t bytes = n64 * slot + (stats ? 2 * (size_t)cap * 4 : 0);
            size_t at[AB_PARTS], len[AB_PARTS], p = 0;
            at[AB_EPOCH] = p; len[AB_EPOCH] = slot; p += slot;
            at[AB_STEP] = p; len[AB_STEP] = slot; p += slot;
            at[AB_STATE] = p; len[AB_STATE] = 13 * slot;
            for (int k = 0; k < 13; ++k) {
                const Part row = arrays_state_row(b, k);
                CHECK(row.at == p && row.bytes == slot, "cap=%lld stats=%d state row %d at %zu (was %zu)", (long long)cap, stats, k, row.at, p);
                p += slot;
            }
            CHECK(arrays_state_bytes(b) == p && p == 15 * slot, "cap=%lld stats=%d: the staged part is %zu bytes (was %zu)", (long long)cap, stats, arrays_state_bytes(b), p);
            for (int k = AB_LAST_STEP; k <= AB_LAST_ERROR; ++k) { at[k] = p; len[k] = stats ? slot : 0; p += len[k]; }
            for (int k = AB_STATUS; k <= AB_LAST_ATTEMPTS; ++k) { at[k] = p; len[k] = stats ? (size_t)cap * 4 : 0; p += len[k]; }
            check_parts(b, at, len, bytes, AB_STATUS, "arrays", cap, stats, 0);
        }
}

static void check_mailbox_block() {
    for (int64_t cap : kCaps) {
        const auto b = mailbox_block(cap);
        // mailbox_acquire of the parent
        const size_t bytes = (size_t)cap * (sizeof(CoopBox) + sizeof(CoopOut)) + 3 * (size_t)(cap + 64) * sizeof(uint32_t);
        // launch_here of the parent: d_coop (CoopBox *), words = (uint32_t *)(d_coop + coop_cap), claimed = words + (coop_cap + 64),
        // finished = words + 2 * (coop_cap + 64), out2 = (CoopOut *)(words + 3 * (coop_cap + 64))
        const size_t words = (size_t)cap * sizeof(CoopBox), set = (size_t)(cap + 64) * sizeof(uint32_t);
        const size_t at[MB_PARTS] = {0, words, words + set, words + 2 * set, words + 3 * set};
        const size_t len[MB_PARTS] = {(size_t)cap * sizeof(CoopBox), set, set, set, (size_t)cap * sizeof(CoopOut)};
        check_parts(b, at, len, bytes, 1, "mailbox", cap, 0, 0);
        // (the scan words the launch clears in one go: from the first to the answers)
        CHECK(b[MB_ANSWERS].at - b[MB_POSTED].at == 3 * (size_t)(cap + 64) * sizeof(uint32_t), "cap=%lld", (long long)cap);
        // a capacity the pool hands out is a multiple of 256: the answers (8-byte granules) are aligned then
        const auto real = mailbox_block(cap_mailbox(cap));
        CHECK(real[MB_ANSWERS].at % 8 == 0 && real[MB_POSTED].at % 64 == 0 && real[MB_CLAIMED].at % 64 == 0 && real[MB_FINISHED].at % 64 == 0, "cap=%lld", (long long)cap_mailbox(cap));
    }
}

static void check_target_keep_block() {
    for (int64_t cap : kCaps) {
        const auto b = target_keep_block(cap);
        // ensure_target_keep and nyx_hip_target_batch_device of the parent: keep = (double *)d_tgt, flag = (int32_t *)(keep + TGT_KEEP_ROWS * cap),
        // active = flag + cap
        const size_t bytes = (size_t)TGT_KEEP_ROWS * (size_t)cap * sizeof(double) + (size_t)cap * sizeof(int32_t) + (NYX_HIP_TARGET_MAX_ITERATIONS + 2) * sizeof(int32_t);
        const size_t keep = (size_t)TGT_KEEP_ROWS * (size_t)cap * sizeof(double);
        const size_t at[TK_PARTS] = {0, keep, keep + (size_t)cap * sizeof(int32_t)};
        const size_t len[TK_PARTS] = {keep, (size_t)cap * sizeof(int32_t), (NYX_HIP_TARGET_MAX_ITERATIONS + 2) * sizeof(int32_t)};
        check_parts(b, at, len, bytes, 1, "target keep", cap, 0, 0);
    }
}

// ---------------------------------------------------------------------------------------------
// the owner, on a counting allocator
// ---------------------------------------------------------------------------------------------
struct Counting {
    static std::map<void *, size_t> live;  // what is allocated, and how large
    static std::vector<std::string> log;   // "alloc", "free", "zero", "quiesce" in the order they happened
    static int allocs, frees, double_frees, fail_next;
    static int alloc(void **p, size_t bytes) {
        if (fail_next) { --fail_next; *p = (void *)0x1; return 2; }  // (a failing allocator may leave anything in *p)
        *p = std::malloc(bytes ? bytes : 1);
        std::memset(*p, 0xa5, bytes);
        live[*p] = bytes;
        ++allocs;
        log.push_back("alloc");
        return 0;
    }
    static void release(void *p) {
        if (!live.count(p)) { ++double_frees; return; }
        live.erase(p);
        std::free(p);
        ++frees;
        log.push_back("free");
    }
    static int zero(void *p, size_t bytes) {
        std::memset(p, 0, bytes);
        log.push_back("zero");
        return 0;
    }
};
std::map<void *, size_t> Counting::live;
std::vector<std::string> Counting::log;
int Counting::allocs = 0, Counting::frees = 0, Counting::double_frees = 0, Counting::fail_next = 0;

static void check_owner() {
    typedef Owned<Counting> Buf;
    int quiesced = 0;
    const auto quiesce = [&] { ++quiesced; Counting::log.push_back("quiesce"); return 0; };
    {
        Buf b;
        CHECK(b.p == nullptr && b.cap == 0, "a new owner is empty");
        // the first block: no quiesce (nothing is held), the rounded capacity, the bytes of that capacity, not zeroed
        CHECK(b.ensure(8, quiesce, cap_batch, PerElement{24}) == 0, "first ensure");
        CHECK(quiesced == 0 && Counting::allocs == 1 && b.cap == 1024 && Counting::live[b.p] == 1024 * 24, "cap %lld", (long long)b.cap);
        CHECK(((unsigned char *)b.p)[0] == 0xa5 && Counting::log == std::vector<std::string>({"alloc"}), "not zeroed");
        // at or below the capacity: the pointer stays, neither the allocator nor quiesce is called
        void *const p0 = b.p;
        for (int64_t n : {1, 8, 1000, 1024}) CHECK(b.ensure(n, quiesce, cap_batch, PerElement{24}) == 0 && b.p == p0 && b.cap == 1024, "n=%lld", (long long)n);
        CHECK(quiesced == 0 && Counting::allocs == 1 && Counting::frees == 0, "no call");
        // growth: quiesce once, before the free; then the allocation, then the zeroing
        Counting::log.clear();
        CHECK(b.ensure(1100, quiesce, cap_batch, PerElement{24}, true) == 0, "growth");
        CHECK(quiesced == 1 && b.cap == 1152 && Counting::live.count(b.p) && Counting::live[b.p] == 1152 * 24, "cap %lld", (long long)b.cap);
        CHECK(Counting::log == std::vector<std::string>({"quiesce", "free", "alloc", "zero"}), "order of a growth");
        CHECK(((unsigned char *)b.p)[0] == 0 && ((unsigned char *)b.p)[1152 * 24 - 1] == 0, "zeroed");
        CHECK(Counting::live.size() == 1, "the old block is gone");
        // a failing allocation: the owner is empty, the error comes back, the old block is freed once
        Counting::fail_next = 1;
        CHECK(b.ensure(5000, quiesce, cap_batch, PerElement{24}) == 2, "failure is reported");
        CHECK(b.p == nullptr && b.cap == 0 && quiesced == 2 && Counting::live.empty(), "empty after a failure");
        // ... and the next call starts over, without quiesce
        CHECK(b.ensure(5000, quiesce, cap_batch, PerElement{24}) == 0 && b.cap == 5056 && quiesced == 2, "after a failure");
        // a quiesce that fails: its code comes back, the block stays
        void *const p1 = b.p;
        CHECK(b.ensure(6000, [] { return 7; }, cap_batch, PerElement{24}) == 7 && b.p == p1 && b.cap == 5056, "failing quiesce");
        // move: the source is empty, the target holds the block; move assignment frees what the target held
        Buf c(std::move(b));
        CHECK(b.p == nullptr && b.cap == 0 && c.p == p1 && c.cap == 5056, "move construction");
        Buf d;
        CHECK(d.ensure(3, quiesce, cap_exact, PerElement{8}) == 0 && d.cap == 3, "exact capacity");
        const int frees = Counting::frees;
        d = std::move(c);
        CHECK(c.p == nullptr && c.cap == 0 && d.p == p1 && d.cap == 5056 && Counting::frees == frees + 1 && Counting::live.size() == 1, "move assignment");
        CHECK(d.as<double>() == (double *)p1, "as");
    }
    // at exit: every allocation freed exactly once
    CHECK(Counting::live.empty() && Counting::allocs == Counting::frees && Counting::double_frees == 0, "%d allocations, %d frees, %d double frees, %zu live",
          Counting::allocs, Counting::frees, Counting::double_frees, Counting::live.size());
}

// ---------------------------------------------------------------------------------------------
// build_run_stream
// ---------------------------------------------------------------------------------------------
// What abi.cpp carried before the function moved (it read ctx->h_cols, ctx->h_tab and ctx->host_cfg.sched): adapted in that only.
struct ParentCtx {
    std::vector<ColHdr> h_cols;
    std::vector<HarmEntry> h_tab;
    const DevCfg &host_cfg;
};
static void parent_build_run_stream(const ParentCtx *ctx, std::initializer_list<int> ids, std::vector<double> &hyb, int64_t &vec_off, std::vector<ColHdr> &cols_x) {
    cols_x = ctx->h_cols;
    std::vector<HarmEntry> t;
    const HarmEntry z = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    std::vector<char> seen(cols_x.size(), 0);
    for (int k : ids) {
        const DevSched &sd = ctx->host_cfg.sched[k];
        for (int w = 0; w < DEV_MAX_WAVES; ++w)
            for (int r = 0; r < sd.n_ranges[w]; ++r) {
                t.resize((t.size() + 15) / 16 * 16, z);
                for (int c = sd.range_c0[w][r]; c < sd.range_c0[w][r] + sd.range_cnt[w][r]; ++c) {
                    if (c < 1 || c >= (int)cols_x.size() || seen[c]) continue;
                    seen[c] = 1;
                    const int32_t src = ctx->h_cols[c].start;
                    cols_x[c].start = (int32_t)t.size();
                    for (int q = 0; q < ctx->h_cols[c].rows; ++q) t.push_back(ctx->h_tab[(size_t)src + q]);
                }
            }
    }
    build_hybrid(t, hyb, vec_off);
}

// row r of a stream in the hybrid layout (build_hybrid)
static HarmEntry stream_row(const std::vector<double> &hyb, int64_t vec_off, size_t r) {
    const double *v = hyb.data() + vec_off + (r / 16) * 64 + r % 16;
    return HarmEntry{hyb[3 * r], hyb[3 * r + 1], hyb[3 * r + 2], v[0], v[16], v[32], v[48]};
}

static int check_streams_of(const char *name, const CtxBuild &b, const DevCfg &dc, const char *plan) {
    const ParentCtx parent{b.cols, b.tab, dc};
    const std::initializer_list<int> id_sets[3] = {{DEV_SCHED_SOLO}, {DEV_SCHED_PRIMARY}, {DEV_SCHED_HELPER, DEV_SCHED_HELPER2}};  // launch_here's three
    int columns = 0;
    for (int s = 0; s < 3; ++s) {
        std::vector<double> hyb, want_hyb;
        std::vector<ColHdr> cols_x, want_cols;
        int64_t vec_off = -1, want_off = -2;
        build_run_stream(b.cols, b.tab, dc.sched, id_sets[s], hyb, vec_off, cols_x);
        parent_build_run_stream(&parent, id_sets[s], want_hyb, want_off, want_cols);
        CHECK(vec_off == want_off && hyb.size() == want_hyb.size() && (hyb.empty() || std::memcmp(hyb.data(), want_hyb.data(), hyb.size() * sizeof(double)) == 0),
              "%s %s set %d: the stream differs from the parent's", name, plan, s);
        CHECK(cols_x.size() == want_cols.size() && (cols_x.empty() || std::memcmp(cols_x.data(), want_cols.data(), cols_x.size() * sizeof(ColHdr)) == 0),
              "%s %s set %d: the column headers differ from the parent's", name, plan, s);
        // every column of the id set once, its rows those of the table; every range at the head of a sixteen-row group
        std::set<int> in_set;
        std::vector<std::pair<size_t, size_t>> pieces;
        for (int k : id_sets[s])
            for (int w = 0; w < DEV_MAX_WAVES; ++w)
                for (int r = 0; r < dc.sched[k].n_ranges[w]; ++r) {
                    bool first = true;
                    for (int c = dc.sched[k].range_c0[w][r]; c < dc.sched[k].range_c0[w][r] + dc.sched[k].range_cnt[w][r]; ++c) {
                        if (c < 1 || c >= (int)b.cols.size() || !in_set.insert(c).second) continue;
                        const size_t at = (size_t)cols_x[c].start, rows = (size_t)b.cols[c].rows;
                        if (first) CHECK(at % 16 == 0, "%s %s set %d: the range of wave %d at column %d begins at row %zu", name, plan, s, w, c, at);
                        first = false;
                        pieces.push_back({at, at + rows});
                        CHECK((int64_t)(3 * (at + rows)) <= vec_off, "%s %s set %d column %d: rows past the stream", name, plan, s, c);
                        for (size_t q = 0; q < rows && (int64_t)(3 * (at + rows)) <= vec_off; ++q) {
                            const HarmEntry got = stream_row(hyb, vec_off, at + q), &want = b.tab[(size_t)b.cols[c].start + q];
                            CHECK(std::memcmp(&got, &want, sizeof got) == 0, "%s %s set %d column %d row %zu", name, plan, s, c, q);
                        }
                    }
                }
        std::sort(pieces.begin(), pieces.end());
        for (size_t k = 1; k < pieces.size(); ++k) CHECK(pieces[k].first >= pieces[k - 1].second, "%s %s set %d: two columns share rows", name, plan, s);
        for (int c = 0; c < (int)b.cols.size(); ++c) {
            if (!in_set.count(c)) CHECK(cols_x[c].start == b.cols[c].start, "%s %s set %d: column %d is not of the set and moved", name, plan, s, c);
            ColHdr a = cols_x[c], o = b.cols[c];
            a.start = o.start = 0;
            CHECK(std::memcmp(&a, &o, sizeof a) == 0, "%s %s set %d column %d: more than `start` changed", name, plan, s, c);
        }
        columns += (int)in_set.size();
    }
    return columns;
}

// the field `degree` x `order` of configs[1]'s force model; `stokes`: [degree, order, C packed, S packed] (nyx_amd/data/*.f64), or null
static void check_field(const char *name, int degree, int order, const std::vector<double> *stokes) {
    std::unique_ptr<lpc::Config> c = lpc::earth_sun_moon(degree);
    c->field[0].order = order;
    if (stokes) {
        const size_t n = (size_t)(degree + 1) * (degree + 2) / 2;
        c->stokes[0].assign(stokes->begin() + 2, stokes->begin() + 2 + n);
        c->stokes[1].assign(stokes->begin() + 2 + n, stokes->begin() + 2 + 2 * n);
        c->field[0].c_nm = c->stokes[0].data();
        c->field[0].s_nm = c->stokes[1].data();
    }
    const nyx_hip_tuning_t tune = NYX_HIP_TUNING_DEFAULT;
    CtxBuild b;
    if (build_context(c->cfg, tune, lpc::lds_room, b) != NYX_HIP_RC_OK) { CHECK(false, "%s: %s", name, b.error.c_str()); return; }
    std::unique_ptr<DevCfg> dc(new DevCfg());
    std::memcpy(dc.get(), &b.dc, sizeof(DevCfg));
    const WeightMap none;
    const PlanInputs in{tune, b.col_len, b.role_handicap, b.terms2, b.ed_reuse_fit, 256, 0, -1, none};
    SchedShape shape;
    // the schedules a context starts with
    plan_first_schedule(in, *dc, shape, b.harm_feed);
    const int first = check_streams_of(name, b, *dc, "first schedule");
    CHECK(first >= dc->n_cols, "%s: the first schedule walks %d of %d columns", name, first, dc->n_cols);
    // ... and, beyond what nyx_hip_ctx_create plans, those of a launch of 10 000 trajectories (cooperative where the planner says so)
    const LaunchPlan p = plan_launch(in, *dc, shape, 10000, true);
    const int launch = check_streams_of(name, b, *dc, "launch of 10000");
    std::printf("%s: %d columns, %d rows; streams of %d columns (first schedule), %d (launch of 10000: %d waves, helpers %s)\n", name, dc->n_cols, (int)b.tab.size(),
                first, launch, p.n_waves, p.coop.run ? "run" : "do not run");
}

int main(int argc, char **argv) {
    if (argc != 2) { std::printf("usage: ctx_mem_check JGM3_70x70_F64\n"); return 2; }
    std::vector<double> jgm3;
    if (std::FILE *f = std::fopen(argv[1], "rb")) {
        double v;
        while (std::fread(&v, sizeof v, 1, f) == 1) jgm3.push_back(v);
        std::fclose(f);
    }
    if (jgm3.size() != 2 + 2 * (71 * 72 / 2) || jgm3[0] != 70.0 || jgm3[1] != 70.0) { std::printf("cannot read a 70x70 field from %s\n", argv[1]); return 2; }
    check_roundings();
    check_arrays_block();
    check_mailbox_block();
    check_target_keep_block();
    check_owner();
    check_field("2x0", 2, 0, nullptr);
    check_field("8x8", 8, 8, nullptr);
    check_field("jgm3 70x70", 70, 70, &jgm3);
    if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
    std::printf("ok\n");
    return 0;
}
