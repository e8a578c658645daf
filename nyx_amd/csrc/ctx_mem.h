// ctx_mem.h - the memory of a context (host only, no HIP; abi.cpp, tests/cxx/ctx_mem_check.cpp): ONE owner of an allocation, ONE rule
// by which it grows, the roundings of the capacities, and the three blocks of a context that hold more than one array (Block<N>,
// dev_block.h): a batch's arrays, the cooperative-mode mailboxes, what the targeter's runs keep between the rounds.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "batch_bind.h"   // kStateRows
#include "dev_block.h"
#include "devcfg.h"       // CoopBox, CoopOut
#include "target_args.h"  // TGT_KEEP_ROWS

// ---- capacities: how many elements a block is given when `n` are asked for
inline int64_t cap_up(int64_t n, int64_t m) { return (n + m - 1) / m * m; }
inline int64_t cap_batch(int64_t n) { return cap_up(std::max<int64_t>(n, 1024), 64); }  // a batch's arrays, the targeter's keep block
inline int64_t cap_stm(int64_t n) { return std::max<int64_t>(n, 1024); }                // the STMs of a batch
inline int64_t cap_stm_hist(int64_t n) { return cap_up(n, 64); }                        // the textbook STM's stage matrices
inline int64_t cap_exact(int64_t n) { return n; }                                       // the swap copy, the run streams, one-off blocks
inline int64_t cap_mailbox(int64_t n) { return cap_up(n, 256); }                        // the cooperative-mode mailboxes

struct PerElement {  // the bytes of a block whose elements are all of one size
    size_t unit;
    size_t operator()(int64_t cap) const { return (size_t)cap * unit; }
};

// ---- the owner: one allocation of `cap` elements, freed with it; move-only.  `Mem` is where the memory comes from:
//   static int alloc(void **p, size_t bytes);  static void release(void *p);  static int zero(void *p, size_t bytes);   (0 = done)
template <typename Mem> struct Owned {
    void *p = nullptr;
    int64_t cap = 0;
    Owned() = default;
    Owned(const Owned &) = delete;
    Owned &operator=(const Owned &) = delete;
    Owned(Owned &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    Owned &operator=(Owned &&o) noexcept {
        if (this != &o) { reset(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    ~Owned() { reset(); }
    void reset() {
        if (p) Mem::release(p);
        p = nullptr; cap = 0;
    }
    template <typename T> T *as() const { return (T *)p; }
    // The grow rule.  Room for `count` elements already: nothing happens, the pointer stays.  Else `quiesce()` - whatever may still
    // use the block has finished; only asked when there is a block -, the block freed, round(count) elements of bytes_of(capacity)
    // bytes allocated and, `zero`, cleared.  A failure (its code is returned; of quiesce: the block stays) leaves the owner empty.
    template <typename Quiesce, typename Bytes>
    int ensure(int64_t count, Quiesce quiesce, int64_t (*round)(int64_t), Bytes bytes_of, bool zero = false) {
        if (cap >= count) return 0;
        if (p)
            if (int e = quiesce()) return e;
        reset();
        const int64_t want = round(count);
        const size_t bytes = bytes_of(want);
        if (int e = Mem::alloc(&p, bytes)) { p = nullptr; return e; }
        if (zero)
            if (int e = Mem::zero(p, bytes)) { reset(); return e; }
        cap = want;
        return 0;
    }
};

// ---- a batch's arrays (DevArrays, abi.cpp): rows of `cap` elements - the epochs, the steps, the thirteen double rows of
// nyx_hip_states_t in header order (kStateRow); `stats`: the five 8-byte rows and the two int32 rows of nyx_hip_step_stats_t
enum { AB_EPOCH, AB_STEP, AB_STATE, AB_LAST_STEP, AB_N_ACC, AB_N_REJ, AB_N_EVALS, AB_LAST_ERROR, AB_STATUS, AB_LAST_ATTEMPTS, AB_PARTS };
inline Block<AB_PARTS> arrays_block(int64_t cap, bool stats) {
    const size_t row = (size_t)cap * 8, stat = stats ? row : 0, words = stats ? (size_t)cap * 4 : 0;
    return Block<AB_PARTS>({row, row, kStateRows * row, stat, stat, stat, stat, stat, words, words});
}
inline Part arrays_state_row(const Block<AB_PARTS> &b, int k) {
    const size_t row = b[AB_STATE].bytes / kStateRows;
    return {b[AB_STATE].at + k * row, row};
}
// what a staged batch uploads: the block up to the end of its state rows
inline size_t arrays_state_bytes(const Block<AB_PARTS> &b) { return b[AB_STATE].at + b[AB_STATE].bytes; }

// ---- the cooperative-mode mailboxes: one box per trajectory-owning workgroup, the three packed scan words (sets of 16 owners:
// <= cap + 16 words each), the answers of part 1 last
enum { MB_BOXES, MB_POSTED, MB_CLAIMED, MB_FINISHED, MB_ANSWERS, MB_PARTS };
inline Block<MB_PARTS> mailbox_block(int64_t cap) {
    const size_t words = (size_t)(cap + 64) * sizeof(uint32_t);
    return Block<MB_PARTS>({(size_t)cap * sizeof(CoopBox), words, words, words, (size_t)cap * sizeof(CoopOut)});
}

// ---- what the targeter's runs keep between the rounds (TgtArgs, target_args.h): keep [TGT_KEEP_ROWS][cap], flag [cap], the runs
// still active after every round
enum { TK_KEEP, TK_FLAG, TK_ACTIVE, TK_PARTS };
inline Block<TK_PARTS> target_keep_block(int64_t cap) {
    return Block<TK_PARTS>({(size_t)TGT_KEEP_ROWS * (size_t)cap * sizeof(double), (size_t)cap * sizeof(int32_t), (NYX_HIP_TARGET_MAX_ITERATIONS + 2) * sizeof(int32_t)});
}
