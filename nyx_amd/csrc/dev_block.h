// dev_block.h - the device block of a host flavour (no HIP, nothing else): byte offsets and sizes of the parts of ONE allocation, in
// the order of the block's enum; an absent part has size 0.  Doubles and int64 first (every such part is a multiple of 8 bytes long),
// the int32 rows last.  The layouts themselves stand beside their family's refusals (run_host.h, series_host.h, stats_host.h,
// lambert_args.h, target_args.h) and are checked on a CPU (tests/cxx/*_host_check.cpp); abi.cpp's host_block allocates and copies them.
#pragma once
#include <cstddef>

struct Part { size_t at = 0, bytes = 0; };
template <int N> struct Block {
    Part part[N];
    size_t total = 0;
    explicit Block(const size_t (&bytes)[N]) { for (int k = 0; k < N; ++k) { part[k] = {total, bytes[k]}; total += bytes[k]; } }
    const Part &operator[](int k) const { return part[k]; }
};
