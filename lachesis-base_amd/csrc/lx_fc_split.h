// lx_fc_split.h -- the column split of a k_root_fc launch (lx_abft_kernels.hip):
// how the launch's tiles divide the padded columns among grid z so that the
// tiles alone need not fill the chip.  Plain C++, tested on the CPU
// (tests/csrc/fc_split_harness.cpp).
#pragma once
#include <cstdint>

struct FcColSplit {
    uint32_t col_split;   // columns per split (a multiple of 32)
    uint32_t n_split;     // splits that hold a column: n_split * col_split >= ncols
};

// tiles: 64 x 64 (candidates x roots) workgroups of the launch, summed over its
// steps; ncols: V rounded up to 32.  Enough splits for 1024 workgroups (256
// CUs x 4), each of at least 4 LDS chunks of 32 columns; rounding the split's
// width up to 32 can leave fewer splits than asked.
inline FcColSplit fc_col_split(uint64_t tiles, uint32_t ncols) {
    const uint64_t max_s = ncols / 128 ? ncols / 128 : 1;
    uint64_t s = tiles ? (1024 + tiles - 1) / tiles : 1;
    s = s < 1 ? 1 : (s > max_s ? max_s : s);
    const uint32_t col_split = (uint32_t)(((ncols + s - 1) / s + 31) / 32 * 32);
    return FcColSplit{col_split, col_split ? (ncols + col_split - 1) / col_split : 0};
}

inline uint64_t fc_tiles(uint32_t n_cand, uint32_t n_roots) {
    return (uint64_t)((n_roots + 63) / 64) * ((n_cand + 63) / 64);
}
