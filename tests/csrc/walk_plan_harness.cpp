// walk_plan_harness.cpp -- CPU test harness of the walk plan
// (lachesis-base_amd/csrc/lx_walk_plan.h): the header's functions over flat C
// structs, for tests/test_walk_plan_cpu.py.  Plain g++, no HIP.  Test
// infrastructure only.
//
// -DWALK_PLAN_MAIN adds a main() that builds the plan of every point of the
// test's grid and checks the seg_map properties the kernel relies on: a
// stand-alone program for a run under the host sanitizers
// (g++ -fsanitize=address,undefined -DWALK_PLAN_MAIN).
#include <cstdio>
#include <cstring>

#include "../../lachesis-base_amd/csrc/lx_walk_plan.h"

extern "C" {

struct wp_in {
    uint32_t ncols, V, B, max_seq, n_cus, sharded, rowseg, crec, cpw, pack16, fold3, seg_xmap, seg_auto, segments;
};
struct wp_out {
    uint32_t cpw, ncw, nd, masked, packed, crec, fold3, n_slices, slices_per_xcd, grid, walk_cus, G, one_launch,
        seg_grid, seg_map_n;
    uint16_t seg_map[256];
};

}  // extern "C"

namespace {

WalkEpoch epoch(const wp_in *i) {
    WalkEpoch e{};
    e.ncols = i->ncols;
    e.V = i->V;
    e.B = i->B;
    e.max_seq = i->max_seq;
    e.n_cus = i->n_cus;
    e.sharded = i->sharded != 0;
    e.rowseg = i->rowseg != 0;
    e.crec = i->crec != 0;
    e.cpw = i->cpw;
    e.pack16 = i->pack16 != 0;
    e.fold3 = i->fold3 != 0;
    e.seg_xmap = i->seg_xmap != 0;
    e.seg_auto = i->seg_auto != 0;
    e.segments = i->segments;
    return e;
}

void flat(const WalkPlan &p, wp_out *o) {
    *o = wp_out{p.cpw,  p.ncw,      p.nd,   p.masked, p.packed,     p.crec,     p.fold3,    p.n_slices, p.slices_per_xcd,
                p.grid, p.walk_cus, p.G,    p.one_launch, p.seg_grid, p.seg_map_n, {}};
    memcpy(o->seg_map, p.seg_map, sizeof o->seg_map);
}

}  // namespace

extern "C" {

// the plan of a batch of n events
void wp_plan(const wp_in *i, uint64_t n, wp_out *o) { flat(walk_plan(epoch(i), n), o); }
// the plan of a walk at a requested width as G segments
void wp_layout(const wp_in *i, uint32_t cpw, uint32_t G, wp_out *o) { flat(walk_layout(epoch(i), cpw, G), o); }
// the segment count and width worth it for n events
uint32_t wp_seg_pick(const wp_in *i, uint64_t n, uint32_t *cpw) { return walk_seg_pick(epoch(i), n, cpw); }
uint32_t wp_crec_ok(const wp_in *i, uint32_t crec_opt) { return walk_crec_ok(epoch(i), crec_opt != 0); }

}  // extern "C"

#ifdef WALK_PLAN_MAIN
namespace {

// every (walk, slice) pair exactly once, idle entries 0xFFFF, <= 256 entries
bool seg_map_ok(const wp_out &o) {
    if (!o.seg_map_n) return true;
    if (o.seg_map_n > 256 || o.seg_map_n != o.seg_grid || o.n_slices > 255) return false;
    std::vector<uint32_t> seen((size_t)o.G * o.n_slices, 0);
    for (uint32_t g = 0; g < o.seg_map_n; g++) {
        const uint16_t m = o.seg_map[g];
        if (m == 0xFFFFu) continue;
        const uint32_t k = m >> 8, sl = m & 0xFFu;
        if (k >= o.G || sl >= o.n_slices || seen[(size_t)k * o.n_slices + sl]++) return false;
    }
    for (uint32_t c : seen)
        if (c != 1) return false;
    return true;
}

}  // namespace

int main() {
    const uint32_t ncols_v[] = {1, 2, 8, 12, 13, 25, 96, 100, 255, 256, 257, 512, 513, 1000, 1021, 3060, 3061};
    const uint32_t seq_v[] = {1, 0x7BFF, 0x7C00, 0xFFFF, 0x10000}, cpw_v[] = {0, 1, 2, 4, 8, 12};
    const uint32_t seg_v[] = {0, 2, 3, 33, 64}, cus_v[] = {64, 256};
    const uint64_t n_v[] = {63, 64, 128, 32767, 65536, 98304, 1ull << 20};
    unsigned long long plans = 0, maps = 0, bad = 0, sum = 0;
    wp_out o;
    for (uint32_t ncols : ncols_v)
        for (uint32_t forks = 0; forks < 2; forks++)
            for (uint32_t seq : seq_v)
                for (uint32_t cpw : cpw_v)
                    for (uint32_t bits = 0; bits < 64; bits++)   // pack16, fold3, crec, seg_xmap, seg_auto, sharded
                        for (uint32_t segs : seg_v)
                            for (uint32_t cus : cus_v) {
                                const wp_in i = {ncols,    ncols,         ncols + 3 * forks, seq,           cus,
                                                 bits >> 5 & 1, 0,        bits >> 2 & 1,     cpw,           bits & 1,
                                                 bits >> 1 & 1, bits >> 3 & 1, bits >> 4 & 1, segs};
                                for (uint64_t n : n_v) {
                                    wp_plan(&i, n, &o);
                                    plans++;
                                    maps += o.seg_map_n != 0;
                                    bad += !seg_map_ok(o);
                                    sum += o.cpw + o.grid + o.seg_grid + o.G;
                                }
                            }
    // the seg_map of every segment count and slice count in range
    for (uint32_t ncols = 1; ncols <= 3072; ncols++)
        for (uint32_t G = 2; G <= kSegLaunchMax; G++) {
            const wp_in i = {ncols, ncols, ncols, 1, 256, 0, 0, 0, 12, 1, 1, 1, 1, 0};
            wp_layout(&i, 12, G, &o);
            plans++;
            maps += o.seg_map_n != 0;
            bad += !seg_map_ok(o);
        }
    printf("walk plans %llu, with a seg_map %llu, bad seg_maps %llu (checksum %llu)\n", plans, maps, bad, sum);
    return bad ? 1 : 0;
}
#endif
