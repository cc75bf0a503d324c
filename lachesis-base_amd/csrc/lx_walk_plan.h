// lx_walk_plan.h -- which walker runs, on what grid: the one place that decides.
//
// The walker (k_index / k_index_segs, lx_kernels.hip) exists in one instance
// per slice width (1, 2, 4, 8, 12 columns per workgroup), masked or not, with
// packed slots, compact records or the three-input fold, as one walk or as G
// Add-order segments side by side.  Everything that picks among them from the
// epoch and the options is here, as pure host functions: plain C++17, no HIP
// types (tests/csrc/walk_plan_harness.cpp compiles it with g++ alone, and
// tests/test_walk_plan_cpu.py checks it against a model of the rules).  The
// callers (lx_index_add.cpp, lx_rowseg.cpp) build one WalkPlan per batch;
// launch_index (lx_kernels.hip) maps it to the kernel and re-decides nothing.
// A new walker variant is added in walk_variant() below and as one line of
// launch_index's table.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

constexpr uint32_t kSegLaunchMax = 32;       // segments of one k_index_segs launch
constexpr uint32_t kFold3MaxSeq = 0x7BFFu;   // the three-input fold's largest seq (pk_max3_f16, lx_internal.h)
constexpr uint64_t kAutoSegEvents = 32768;   // events per side-by-side segment, at least
// pass cost of a slice width against 1-column slices, as measured: 1-, 2- and
// 4-column slices on C2 (1, 1.15, 1.28)
constexpr float kPass12 = 2.1f;  // 12-column slices (C3: three walks 50.0 ms vs two 8-column walks 61.2 ms -> 1.7 x 3 / 2 x 50.0 / 61.2)
constexpr float kPass8 = 1.7f;   // pass cost of 8- vs 1-column slices (8 compute + 7 drain waves; C3 one walk: 121.7 ms at 8 columns, 91.4 at 4 = 1.28)

// The epoch as the next walk finds it, and the options (lx_set_option)
struct WalkEpoch {
    uint32_t ncols;      // columns to walk (a shard: its own)
    uint32_t V, B;       // validators, branches (B > V: forks, older rows may carry fork marks)
    uint32_t max_seq;    // largest seq of the epoch so far
    uint32_t n_cus;      // compute units of the device
    bool sharded;        // column shard (the walk maps branches to plane columns)
    bool rowseg;         // row-segment rank
    bool crec;           // compact records were written for this batch (walk_crec_ok)
    uint32_t cpw;        // option cpw: columns per workgroup, 0 = default
    bool pack16, fold3, seg_xmap, seg_auto;   // the options of these names
    uint32_t segments;   // option segments
};

// Everything a launch needs and nothing the device reads
struct WalkPlan {
    // the kernel instance
    uint32_t cpw;        // columns per workgroup: 1, 2, 4, 8 or 12
    uint32_t ncw, nd;    // compute and drain waves (+ 1 loader wave)
    bool masked, packed, crec, fold3;
    // one walk
    uint32_t n_slices, slices_per_xcd;
    uint32_t grid;       // workgroups of one walk's launch (whole XCD rounds)
    uint32_t walk_cus;   // CUs one walk holds
    // G > 0: the batch as G Add-order segments, by one launch side by side
    // (one_launch, seg_grid workgroups) or one walk after the other
    uint32_t G;
    bool one_launch;
    uint32_t seg_grid;
    // 12-column side-by-side walks under option seg_xmap: workgroup -> (walk
    // << 8 | slice), 0xFFFF idle; seg_map_n = 0: the kernel's seg_chunk mapping
    uint32_t seg_map_n;
    uint16_t seg_map[256];
};

// every seq of the epoch fits 16 bits: one 16-B slot unit per event
inline bool walk_packed(const WalkEpoch &e) { return e.pack16 && e.max_seq <= 0xFFFFu; }
// 8- and 12-column slices: packed 16-bit slots only (every seq <= 0xFFFF, no forks)
inline bool walk_wide_ok(const WalkEpoch &e) { return walk_packed(e) && e.B <= e.V; }
// compact records (option crec) are written beside the full ones for the 8- /
// 12-column walks: fork-free epoch, every branch and seq within 16 bits
inline bool walk_crec_ok(const WalkEpoch &e, bool crec_opt) { return crec_opt && walk_wide_ok(e) && e.B <= 0xFFFFu; }

// The kernel instance and one walk's grid for a requested width (0: the
// default).  Columns per workgroup: the fewest that still leave at most ~256
// workgroups (one per CU); the pass gets shorter with fewer columns per slice,
// and the walk time is levels x pass latency whatever the number of
// workgroups.  Compute waves: 8 on 1- / 2-column slices (11 slowed C2 by 7 %),
// 11 on 4-column slices (16 waves with the loader and 4 drains, the workgroup
// limit: C3 walk -1.8 % against 8).  8 and 12 columns (V = 1000: 84 slices,
// three walks side by side on 256 CUs): twice the drains' work per event (HB
// row, range fills), so 7 drain waves beside 8 compute waves.
inline void walk_variant(const WalkEpoch &e, uint32_t cpw, WalkPlan *p) {
    if (!cpw) cpw = e.ncols <= 256 ? 1 : e.ncols <= 512 ? 2 : 4;
    if (cpw >= 8 && !walk_wide_ok(e)) cpw = 4;
    if (cpw == 12 && e.sharded) cpw = 8;   // 12-column slices use the identity column map
    p->cpw = cpw <= 1 ? 1 : cpw <= 2 ? 2 : cpw == 8 || cpw == 12 ? cpw : 4;
    const bool wide = p->cpw >= 8;
    p->ncw = p->cpw == 4 ? 11 : 8;
    p->nd = wide ? 7 : 4;
    p->masked = e.B > e.V;
    p->packed = p->cpw >= 4 && walk_packed(e);
    p->crec = wide && e.crec;
    // (the three-input fold: full records only)
    p->fold3 = wide && !p->crec && e.fold3 && e.max_seq <= kFold3MaxSeq;
    p->n_slices = (e.ncols + p->cpw - 1) / p->cpw;
    p->slices_per_xcd = (p->n_slices + 7) / 8;
    p->grid = p->slices_per_xcd * 8;
    // the CUs a walk holds: 12-column slices count only the real slices (the
    // launch's rounding workgroups leave at once and free their CUs for the
    // next walk's: V = 1000, 84 slices, three walks side by side)
    p->walk_cus = p->cpw == 12 ? p->n_slices : p->grid;
}

// Option seg_xmap (12-column side-by-side walks): groups of 8 slices (96
// columns = three 128-B HB lines) stay on one XCD, so every HB line is
// assembled in one L2; whole groups go round-robin to the least-loaded XCD,
// the short last group of each walk after them
inline void walk_seg_map(WalkPlan *p) {
    std::vector<std::vector<uint16_t>> xl(8);
    auto put = [&](uint32_t k, uint32_t s0, uint32_t cnt) {
        uint32_t x = 0;
        for (uint32_t y = 1; y < 8; y++)
            if (xl[y].size() < xl[x].size()) x = y;
        for (uint32_t s = s0; s < s0 + cnt; s++) xl[x].push_back((uint16_t)(k << 8 | s));
    };
    for (uint32_t k = 0; k < p->G; k++)
        for (uint32_t s0 = 0; s0 + 8 <= p->n_slices; s0 += 8) put(k, s0, 8);
    if (p->n_slices % 8)
        for (uint32_t k = 0; k < p->G; k++) put(k, p->n_slices / 8 * 8, p->n_slices % 8);
    size_t mx = 0;
    for (auto &l : xl) mx = std::max(mx, l.size());
    if (8 * mx <= 256 && 8 * mx <= p->seg_grid + 8) {
        p->seg_map_n = (uint32_t)(8 * mx);
        for (uint32_t g = 0; g < p->seg_map_n; g++)
            p->seg_map[g] = g / 8 < xl[g % 8].size() ? xl[g % 8][g / 8] : (uint16_t)0xFFFFu;
        p->seg_grid = p->seg_map_n;
    }
}

// The plan of a walk at the requested width, as G Add-order segments (G < 2:
// one walk): one launch for all G when they fit the CUs side by side (one
// workgroup per CU each), otherwise one walk after the other
inline WalkPlan walk_layout(const WalkEpoch &e, uint32_t cpw, uint32_t G) {
    WalkPlan p{};
    walk_variant(e, cpw, &p);
    p.G = G >= 2 ? G : 0;
    p.one_launch = p.G && p.G <= kSegLaunchMax && p.G * p.walk_cus <= e.n_cus;
    if (!p.one_launch) return p;
    // 12 columns: workgroup g runs on XCD g % 8, which takes a chunk of each
    // walk's slices in turn: at most ceil(G * slices / 8) workgroups per XCD
    // (seg_chunk, lx_kernels.hip); otherwise grid-sized blocks of workgroups
    p.seg_grid = p.cpw == 12 ? 8 * (p.G * (p.n_slices / 8) + (p.G * (p.n_slices % 8) + 7) / 8) : p.grid * p.G;
    if (p.cpw == 12 && e.seg_xmap && p.n_slices <= 255) walk_seg_map(&p);
    return p;
}

// Segments walked at once on idle compute units: a walk of few columns leaves
// most CUs idle (C2: 100 columns, 104 workgroups on 256 CUs), and its time is
// the batch's DAG depth x pass latency, so G concurrent Add-order segments
// walk ~1/G of the levels each.  Wider slices free more CUs for more segments
// at a longer pass (kPass*): the slice width with the smallest pass / G wins.
// The segment count for n events, 0 when they stay one walk; *cpw = the width
// (row-segment ranks split their own segment by it too, lx_rowseg.cpp).
inline uint32_t walk_seg_pick(const WalkEpoch &e, uint64_t n, uint32_t *cpw) {
    static const float kPass[13] = {0, 1.0f, 1.15f, 0, 1.28f, 0, 0, 0, kPass8, 0, 0, 0, kPass12};
    uint32_t best_g = 0;
    float best = 1.0f;   // one walk at the default width
    for (uint32_t c : {1u, 2u, 4u, 8u, 12u}) {
        if ((e.cpw && c != e.cpw) || (c >= 8 && !walk_wide_ok(e))) continue;
        WalkPlan p{};
        walk_variant(e, c, &p);
        uint32_t G = std::min<uint32_t>(e.n_cus / p.walk_cus, kSegLaunchMax);
        while (G >= 2 && n < (uint64_t)G * kAutoSegEvents) G--;
        if (G >= 2 && kPass[c] / G < best) {
            best = kPass[c] / G;
            best_g = G;
            *cpw = c;
        }
    }
    return best_g;
}

// The plan of a batch of n events: option segments (each >= 64 events; above
// kSegLaunchMax one walk after the other), else the segments walk_seg_pick
// finds worth it, else one walk at option cpw.  Column shards and row-segment
// ranks never split here (a rank splits its own segment, lx_rowseg.cpp).
inline WalkPlan walk_plan(const WalkEpoch &e, uint64_t n) {
    if (e.segments > 1 && !e.sharded && !e.rowseg && n >= 64ull * e.segments) return walk_layout(e, e.cpw, e.segments);
    uint32_t cpw = e.cpw, G = 0;
    if (e.seg_auto && !e.sharded && !e.rowseg && e.segments <= 1 && e.ncols) G = walk_seg_pick(e, n, &cpw);
    return walk_layout(e, G ? cpw : e.cpw, G);
}
