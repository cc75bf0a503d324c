// fc_split_harness.cpp -- CPU test harness of the root-FC column split
// (lachesis-base_amd/csrc/lx_fc_split.h) for tests/test_fc_split_cpu.py.
// Plain g++, no HIP.  Test infrastructure only.
#include "../../lachesis-base_amd/csrc/lx_fc_split.h"

extern "C" {

void fs_col_split(uint64_t tiles, uint32_t ncols, uint32_t *col_split, uint32_t *n_split) {
    const FcColSplit sp = fc_col_split(tiles, ncols);
    *col_split = sp.col_split;
    *n_split = sp.n_split;
}

uint64_t fs_tiles(uint32_t n_cand, uint32_t n_roots) { return fc_tiles(n_cand, n_roots); }

}  // extern "C"
