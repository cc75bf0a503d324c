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
//   k_anc_fork    : fork evidence, one wave per (head, creator) query: the
//                   pair of events behind a cheater flag (see there).
//   No kernel waits for another workgroup.
// Integer gathers; bound by the launches at the sizes of one epoch.
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "../../include/lachesis_ancestry.h"
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

// ---- fork evidence: the two events behind a cheater flag
//
// A branch is a chain of consecutive seqs and "head observes its k-th event"
// is monotone in k, so head's view of branch b is an interval of seqs
// [first_b, hi_b] (or nothing), hi_b found by a binary search over brow[b] with
// the LowestAfter rule (the HighestBefore entries of a detected cheater are
// all marks and say nothing).  The lowest seq two intervals share is a first
// seq: seq* = min { first_j : some i != j has first_i <= first_j <= hi_i }
// (below the start of both intervals that cover it a shared seq would have a
// shared predecessor).  The pair: the two lowest events brow[b][seq* - first_b]
// over the intervals that hold seq*.
//
// One wave per query; a lane takes the creator's branches lane, lane + 64, ..
// of the CSR, the lanes' searches run in lockstep.  The intervals stay in LDS
// (kAncForkMaxBr per wave, checked by the host).
__global__ __launch_bounds__(kAncThreads) void k_anc_fork(AncForkArgs a) {
    __shared__ uint32_t sFirst[kAncForkWaves][kAncForkMaxBr], sHi[kAncForkWaves][kAncForkMaxBr];
    const uint32_t lane = threadIdx.x % 64, wave = threadIdx.x / 64;
    const uint64_t q = (uint64_t)blockIdx.x * kAncForkWaves + wave;
    uint32_t h = 0, c = 0;
    int32_t k = -1;
    if (q < a.n) {
        if (a.creator) {
            h = a.head[q];
            c = a.creator[q];
        } else {
            h = a.head[q / a.n_cheat];
            c = a.cheat_creator[q % a.n_cheat];
        }
        k = a.cheat_of[c];
        // marks are per creator: head has not detected the fork where its entry
        // of the creator's original branch (column c) is no mark
        if (k >= 0 && !(a.hb[(uint64_t)h * a.stride + c] & LX_MARK)) k = -1;
    }
    uint32_t rx = LX_ANC_NONE, ry = LX_ANC_NONE, rs = 0;
    uint32_t o0 = 0, nb = 0, seen = 0;   // seen: branches head observes, of this lane
    uint32_t *first = sFirst[wave], *hi = sHi[wave];
    if (k >= 0) {   // (the same in every lane of the wave)
        o0 = a.cheat_off[k];
        nb = a.cheat_off[k + 1] - o0;
        nb = nb < kAncForkMaxBr ? nb : kAncForkMaxBr;   // (the host refused more)
        const uint32_t hbr = a.ev_branch[h], hs = a.ev_seq[h];
        for (uint32_t j = lane; j < nb; j += 64) {
            const uint32_t b = a.cheat_br[o0 + j];
            const uint32_t *row = a.brow + (uint64_t)b * a.s_cap;
            uint32_t lo = 0, up = a.branch_len[b];
            up = up < a.s_cap ? up : a.s_cap;
            while (lo < up) {   // events [0, lo) are observed, [up, len) are not
                const uint32_t mid = (lo + up) / 2, x = row[mid];
                if (x <= h && anc_marked_observes(a.la, a.stride, x, hbr, hs)) lo = mid + 1;
                else up = mid;
            }
            const uint32_t f = a.branch_first[b];
            first[j] = lo ? f : LX_ANC_NONE;
            hi[j] = lo ? f + lo - 1 : 0;
            seen += lo != 0;
        }
    }
    __syncthreads();   // a wave reads the intervals its other lanes wrote
    if (k >= 0) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) seen += __shfl_xor(seen, off, 64);
        if (seen >= 2) {
            uint32_t best = LX_ANC_NONE;
            for (uint32_t j = lane; j < nb; j += 64) {
                const uint32_t f = first[j];
                if (f == LX_ANC_NONE || f >= best) continue;
                for (uint32_t i = 0; i < nb; i++)
                    if (i != j && first[i] <= f && f <= hi[i]) {
                        best = f;
                        break;
                    }
            }
            best = wave_min_u32(best);
            if (best != LX_ANC_NONE) {
                uint32_t m1 = LX_ANC_NONE, m2 = LX_ANC_NONE;   // the two lowest events of this lane
                for (uint32_t j = lane; j < nb; j += 64) {
                    if (first[j] > best || best > hi[j]) continue;
                    const uint32_t b = a.cheat_br[o0 + j];
                    const uint32_t e = a.brow[(uint64_t)b * a.s_cap + (best - first[j])];
                    if (e < m1) m2 = m1, m1 = e;
                    else if (e < m2) m2 = e;
                }
                const uint32_t w1 = wave_min_u32(m1);
                const uint32_t w2 = wave_min_u32(m1 == w1 ? m2 : m1);   // (events are distinct)
                rx = w1, ry = w2, rs = best;
            }
        }
    }
    if (lane == 0 && q < a.n) {
        a.x[q] = rx;
        a.y[q] = ry;
        a.seq[q] = rs;
    }
}

__global__ __launch_bounds__(kAncThreads) void k_anc_fork_flag(AncForkListArgs a, uint64_t n) {
    const uint64_t q = (uint64_t)blockIdx.x * kAncThreads + threadIdx.x;
    if (q <= n) a.flag[q] = q < n && a.x[q] != LX_ANC_NONE;
}

__global__ __launch_bounds__(kAncThreads) void k_anc_fork_scatter(AncForkListArgs a, uint64_t n) {
    const uint64_t q = (uint64_t)blockIdx.x * kAncThreads + threadIdx.x;
    if (q < a.n_heads) a.n_found[q] = a.off[(q + 1) * a.n_cheat] - a.off[q * a.n_cheat];
    if (q >= n || !a.flag[q]) return;
    const uint64_t pos = a.base + a.off[q];
    a.out_creator[pos] = a.cheat_creator[q % a.n_cheat];
    a.out_x[pos] = a.x[q];
    a.out_y[pos] = a.y[q];
    a.out_seq[pos] = a.seq[q];
}

}  // namespace

hipError_t launch_anc_fork(const AncForkArgs &a, hipStream_t s) {
    if (!a.n) return hipSuccess;
    const uint64_t blocks = (a.n + kAncForkWaves - 1) / kAncForkWaves;
    if (blocks > 0x7FFFFFFFull || (!a.creator && !a.n_cheat)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_anc_fork, dim3((uint32_t)blocks), dim3(kAncThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_anc_fork_list(const AncForkListArgs &a, void *tmp, size_t tmp_bytes, hipStream_t s) {
    const uint64_t n = (uint64_t)a.n_heads * a.n_cheat;
    if (!n) return hipSuccess;
    if (n + 1 > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const dim3 grid((uint32_t)((n + 1 + kAncThreads - 1) / kAncThreads)), block(kAncThreads);
    hipLaunchKernelGGL(k_anc_fork_flag, grid, block, 0, s, a, n);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    size_t tb = tmp_bytes;
    e = hipcub::DeviceScan::ExclusiveSum(tmp, tb, a.flag, a.off, (int)(n + 1), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_anc_fork_scatter, grid, block, 0, s, a, n);
    return hipGetLastError();
}

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
