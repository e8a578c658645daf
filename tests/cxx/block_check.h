// A device block (nyx_amd/csrc/dev_block.h) against what abi.cpp computed inline before a header had the layout, restated by the
// caller: every part where and as large as it was, in order and not overlapping, the total the size of the allocation, the first
// `n_f64` parts (doubles, int64) at multiples of 8 and the int32 parts behind them at multiples of 4.  The including program defines
// CHECK(cond, format, ...).
#pragma once
#include <cstddef>

#include "../../nyx_amd/csrc/dev_block.h"

template <int N> static void check_parts(const Block<N> &b, const size_t (&at)[N], const size_t (&bytes)[N], size_t total, int n_f64, const char *what, long long n, int p, int q) {
    size_t end = 0;
    for (int k = 0; k < N; ++k) {
        CHECK(b[k].at == at[k] && b[k].bytes == bytes[k], "%s n=%lld (%d, %d) part %d: at %zu, %zu bytes (was at %zu, %zu bytes)", what, n, p, q, k, b[k].at, b[k].bytes, at[k], bytes[k]);
        CHECK(b[k].at == end, "%s n=%lld (%d, %d) part %d: begins at %zu, the part before it ends at %zu", what, n, p, q, k, b[k].at, end);
        CHECK(b[k].at % (k < n_f64 ? 8 : 4) == 0, "%s n=%lld (%d, %d) part %d: at %zu", what, n, p, q, k, b[k].at);
        end = b[k].at + b[k].bytes;
    }
    CHECK(b.total == total && b.total == end, "%s n=%lld (%d, %d): total %zu, allocated were %zu, the parts end at %zu", what, n, p, q, b.total, total, end);
}
