// lx_ancestry.hip -- CDNA4 (gfx950) kernels of include/lachesis_ancestry.h:
// "x is head or an ancestor of head" read from the planes, no parent list.
//
//   observes(head, x), x <= head (an event above head is never its ancestor):
//     e = hb[head][branch(x)]
//     e unmarked : seq(e) >= seq(x)      (a branch is a chain of consecutive
//                  seqs, and the entry is the highest seq of it head observes)
//     e marked   : 0 < la[x][branch(head)] <= seq(head)   (head sees branch(x)'s
//                  creator as a cheater and the entry says no more; LowestAfter
//                  is set by the reference's DFS whatever the marks)
//
//   k_anc_pairs   : one thread per (head, x) pair.
//   k_anc_count   : one confirm launch of up to kAncMaxHeads heads over the
//                   events [lo, hi).  A workgroup stages the heads' HB rows in
//                   LDS (at most kAncLdsBytes), streams ev_branch / ev_seq /
//                   labels of its per_wg events coalesced and reads the LA
//                   column only where the entry is marked.  Per event the
//                   first head in call order that observes it (win), per
//                   workgroup and head their number (cnt), and the lowest
//                   event left without a label (atomicMin).
//   (one exclusive scan of cnt, head-major: the place of every (head,
//    workgroup) group in the ordered output)
//   k_anc_scatter : writes the labels and the events, a wave-ballot prefix
//                   inside the workgroup keeps a group in ascending order.
//   No kernel waits for another workgroup.
// Integer gathers; bound by the launches at the sizes of one epoch.
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "lx_internal.h"

namespace lx {

namespace {

constexpr uint32_t kAncWaves = kAncThreads / 64;

__device__ __forceinline__ bool anc_marked_observes(const uint32_t *la, uint64_t stride, uint32_t x, uint32_t hbranch,
                                                    uint32_t hseq) {
    const uint32_t l = la[(uint64_t)x * stride + hbranch];
    return l != 0 && l <= hseq;
}

__global__ __launch_bounds__(kAncThreads) void k_anc_pairs(AncPairArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * kAncThreads + threadIdx.x;
    if (i >= a.n) return;
    const uint32_t h = a.head[i], x = a.x[i];
    uint8_t r;
    if (x >= h) {
        r = x == h;
    } else {
        const uint32_t e = a.hb[(uint64_t)h * a.stride + a.ev_branch[x]];
        if (e & LX_MARK) r = anc_marked_observes(a.la, a.stride, x, a.ev_branch[h], a.ev_seq[h]);
        else r = e >= a.ev_seq[x];
    }
    a.out[i] = r;
}

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t y = __shfl_xor(x, off, 64);
        x = y < x ? y : x;
    }
    return x;
}

// events of workgroup wg: [first, first + m)
__device__ __forceinline__ uint32_t anc_tile(const AncArgs &a, uint32_t wg, uint32_t *first) {
    *first = a.lo + wg * a.per_wg;
    const uint32_t left = a.hi - *first;
    return left < a.per_wg ? left : a.per_wg;
}

template <bool VEC>
__global__ __launch_bounds__(kAncThreads) void k_anc_count(AncArgs a) {
    extern __shared__ uint4 sRows4[];
    uint32_t *sRows = (uint32_t *)sRows4;
    __shared__ uint32_t sHead[kAncMaxHeads], sHb[kAncMaxHeads], sHs[kAncMaxHeads], sCnt[kAncMaxHeads], sMin;
    const uint32_t tid = threadIdx.x, wg = blockIdx.x;
    uint32_t first;
    const uint32_t m = anc_tile(a, wg, &first);
    if (tid < kAncMaxHeads) {
        sCnt[tid] = 0;
        if (tid < a.H) {
            const uint32_t h = a.head[tid];
            sHead[tid] = h;
            sHb[tid] = a.ev_branch[h];
            sHs[tid] = a.ev_seq[h];
        }
    }
    if (tid == 0) sMin = LX_NONE;
    const bool ask = first <= a.top;   // else every event of the tile lies above every head
    if (ask) {
        for (uint32_t k = 0; k < a.H; k++) {
            const uint32_t *row = a.hb + (uint64_t)a.head[k] * a.stride;
            if (VEC) {   // stride % 4 == 0: the row is 16-B aligned and row_words <= stride
                const uint4 *row4 = (const uint4 *)row;
                uint4 *dst = sRows4 + (size_t)k * (a.row_words / 4);
                for (uint32_t j = tid; j < a.row_words / 4; j += kAncThreads) dst[j] = row4[j];
            } else {
                uint32_t *dst = sRows + (size_t)k * a.row_words;
                for (uint32_t j = tid; j < a.B; j += kAncThreads) dst[j] = row[j];
            }
        }
    }
    __syncthreads();
    uint32_t mn = LX_NONE;
    for (uint32_t i = tid; i < m; i += kAncThreads) {
        const uint32_t e = first + i;
        uint32_t w = kAncNoHead;
        if (a.labels[e] == 0) {
            if (ask && e <= a.top) {
                const uint32_t br = a.ev_branch[e], sq = a.ev_seq[e];
                if (br < a.B) {
                    for (uint32_t k = 0; k < a.H; k++) {
                        if (e > sHead[k]) continue;
                        const uint32_t ent = sRows[(size_t)k * a.row_words + br];
                        const bool obs = (ent & LX_MARK) ? anc_marked_observes(a.la, a.stride, e, sHb[k], sHs[k])
                                                         : ent >= sq;
                        if (obs) {
                            w = k;
                            break;
                        }
                    }
                }
            }
            if (w == kAncNoHead) mn = e < mn ? e : mn;
        }
        a.win[e - a.lo] = (uint8_t)w;
        if (w != kAncNoHead) atomicAdd(&sCnt[w], 1u);
    }
    mn = wave_min_u32(mn);
    if (tid % 64 == 0 && mn != LX_NONE) atomicMin(&sMin, mn);
    __syncthreads();
    if (tid < a.H) a.cnt[1 + (size_t)tid * a.n_wg + wg] = sCnt[tid];
    if (tid == 0) {
        if (sMin != LX_NONE) atomicMin(a.low, sMin);
        if (wg == 0) a.cnt[1 + (size_t)a.H * a.n_wg] = 0;
    }
}

__global__ __launch_bounds__(kAncThreads) void k_anc_scatter(AncArgs a) {
    __shared__ uint32_t sRun[kAncMaxHeads], sLab[kAncMaxHeads], sW[kAncWaves][kAncMaxHeads];
    const uint32_t tid = threadIdx.x, wg = blockIdx.x, lane = tid % 64, wave = tid / 64;
    uint32_t first;
    const uint32_t m = anc_tile(a, wg, &first);
    if (tid < a.H) {
        sRun[tid] = a.off[1 + (size_t)tid * a.n_wg + wg];
        sLab[tid] = a.label[tid];
        if (wg == 0) a.n_new[tid] = a.off[1 + (size_t)(tid + 1) * a.n_wg] - a.off[1 + (size_t)tid * a.n_wg];
    }
    // the next launch of the call continues the output where this one ends
    // (cnt is the scan's input: nothing of this launch reads it any more)
    if (wg == 0 && tid == 0) a.cnt[0] = a.off[1 + (size_t)a.H * a.n_wg];
    __syncthreads();
    for (uint32_t i0 = 0; i0 < m; i0 += kAncThreads) {
        const uint32_t i = i0 + tid;
        const uint32_t w = i < m ? a.win[first - a.lo + i] : kAncNoHead;
        if (!__syncthreads_or(w != kAncNoHead)) continue;   // (the same answer in every thread)
        uint32_t rank = 0;
        for (uint32_t k = 0; k < a.H; k++) {
            const unsigned long long mask = __ballot(w == k);
            if (lane == 0) sW[wave][k] = (uint32_t)__popcll(mask);
            if (w == k) rank = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
        }
        __syncthreads();
        if (w != kAncNoHead) {
            uint32_t pos = sRun[w] + rank;
            for (uint32_t v = 0; v < wave; v++) pos += sW[v][w];
            const uint32_t e = first + i;
            if (pos < a.out_cap) a.out_ev[pos] = e;
            a.labels[e] = sLab[w];
        }
        __syncthreads();
        if (tid < a.H) {
            uint32_t s = 0;
            for (uint32_t v = 0; v < kAncWaves; v++) s += sW[v][tid];
            sRun[tid] += s;
        }
        __syncthreads();
    }
}

// the lowest event of [lo, hi) without a label
__global__ __launch_bounds__(kAncThreads) void k_anc_low(const uint32_t *labels, uint32_t lo, uint32_t hi, uint32_t *low) {
    uint32_t mn = LX_NONE;
    const uint64_t step = (uint64_t)gridDim.x * kAncThreads;
    for (uint64_t e = lo + (uint64_t)blockIdx.x * kAncThreads + threadIdx.x; e < hi; e += step)
        if (labels[e] == 0 && (uint32_t)e < mn) mn = (uint32_t)e;
    mn = wave_min_u32(mn);
    if (threadIdx.x % 64 == 0 && mn != LX_NONE) atomicMin(low, mn);
}

}  // namespace

hipError_t launch_anc_pairs(const AncPairArgs &a, hipStream_t s) {
    if (!a.n) return hipSuccess;
    const uint64_t blocks = (a.n + kAncThreads - 1) / kAncThreads;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_anc_pairs, dim3((uint32_t)blocks), dim3(kAncThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t anc_scan_bytes(uint32_t n, size_t *bytes) {
    return hipcub::DeviceScan::ExclusiveSum(nullptr, *bytes, (uint32_t *)nullptr, (uint32_t *)nullptr, (int)n);
}

hipError_t launch_anc_confirm(const AncArgs &a, void *tmp, size_t tmp_bytes, hipStream_t s) {
    if (a.hi <= a.lo) return hipSuccess;
    const bool vec = a.stride % 4 == 0;
    const size_t lds = (size_t)a.H * a.row_words * 4;
    if (!a.H || a.H > kAncMaxHeads || lds > kAncLdsBytes || !a.n_wg || a.per_wg % kAncThreads ||
        (uint64_t)a.n_wg * a.per_wg < (uint64_t)(a.hi - a.lo) || a.row_words < a.B || (vec && a.row_words % 4) ||
        a.row_words > a.stride)
        return hipErrorInvalidValue;
    const dim3 grid(a.n_wg), block(kAncThreads);
    if (vec) hipLaunchKernelGGL(k_anc_count<true>, grid, block, lds, s, a);
    else hipLaunchKernelGGL(k_anc_count<false>, grid, block, lds, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    size_t tb = tmp_bytes;
    e = hipcub::DeviceScan::ExclusiveSum(tmp, tb, a.cnt, a.off, (int)(2 + a.H * a.n_wg), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_anc_scatter, grid, block, 0, s, a);
    return hipGetLastError();
}

hipError_t launch_anc_low(const uint32_t *labels, uint32_t lo, uint32_t hi, uint32_t *low, hipStream_t s) {
    if (hi <= lo) return hipSuccess;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(((uint64_t)(hi - lo) + kAncThreads - 1) / kAncThreads, 1024);
    hipLaunchKernelGGL(k_anc_low, dim3(blocks), dim3(kAncThreads), 0, s, labels, lo, hi, low);
    return hipGetLastError();
}

}  // namespace lx
