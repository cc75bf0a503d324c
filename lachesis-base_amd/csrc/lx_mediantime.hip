// lx_mediantime.hip -- CDNA4 (gfx950) kernel of MedianTime
// (include/lachesis_mediantime.h) on the index's HighestBefore plane.
//
//   k_mt<E> : one workgroup per queried event e, E validators per thread held
//             in registers (v = tid + u * blockDim.x: the row is read
//             coalesced).
//     gather  the merged entry of validator v (GetMergedHighestBefore,
//             vecengine/index.go:235-250 with GatherFrom, vecfc/vector_ops.go:
//             81-96; marks are per creator, so the mark of column v decides,
//             as merged_seq in lx_emitter.hip) gives the winning (branch,
//             seq); brow names the one event at that place, `times` its
//             creation time: two dependent loads, no time plane.
//     median  no sort: with half = honest / 2 > 0 the answer is the smallest
//             t whose weight at or below t reaches half, found bit by bit from
//             the highest bit in which two weighted times differ (the common
//             prefix above it is given) -- one block sum per bit, the entries
//             never leave their registers.  half = 0 returns the smallest
//             time of all V pairs, the cheaters' zeros included.
// Integer work on one row per event; latency-bound.
#include "lx_internal.h"

namespace lx {

namespace {

constexpr uint32_t kMtWaves = kMtThreads / 64;

__device__ __forceinline__ uint32_t wave_sum(uint32_t x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
    return x;
}
__device__ __forceinline__ unsigned long long wave_min(unsigned long long x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long y = __shfl_xor(x, off, 64);
        x = y < x ? y : x;
    }
    return x;
}
__device__ __forceinline__ unsigned long long wave_max(unsigned long long x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long y = __shfl_xor(x, off, 64);
        x = y > x ? y : x;
    }
    return x;
}

// merged entry of validator v in HB row `row`: 0 = fork detected, 1 =
// unobserved, 2 = observed with *t its time
__device__ __forceinline__ uint32_t merged_time(const MtArgs &a, const uint32_t *row, uint32_t v,
                                                unsigned long long *t) {
    *t = 0;
    uint32_t s = row[v], b = v;
    if (a.forks) {
        if (s & LX_MARK) return 0;
        const int32_t k = a.cheat_of[v];
        if (k >= 0) {
            s = 0;
            for (uint32_t o = a.cheat_off[k]; o < a.cheat_off[k + 1]; o++) {
                const uint32_t br = a.cheat_br[o], x = row[br] & LX_SEQ_MASK;
                if (x > s) s = x, b = br;   // the first strictly greatest
            }
        }
    }
    if (!s) return 1;
    // (branch, seq) -> event -> time; what the tables cannot hold reads as 0
    const uint32_t k = s - a.branch_first[b];
    if (k < a.s_cap) {
        const uint32_t x = a.brow[(uint64_t)b * a.s_cap + k];
        if (x < a.n_times) *t = a.times[x];
    }
    return 2;
}

template <uint32_t E>
__global__ __launch_bounds__(kMtThreads) void k_mt(MtArgs a) {
    __shared__ uint32_t sHonest[kMtWaves], sW[2][kMtWaves];
    __shared__ unsigned long long sAll[kMtWaves], sLo[kMtWaves], sHi[kMtWaves];
    const uint32_t i = blockIdx.x, tid = threadIdx.x, T = blockDim.x, nw = T / 64, wave = tid / 64;
    const uint32_t e = a.ev ? a.ev[i] : a.iev[i];
    const uint32_t *row = a.hb + (uint64_t)e * a.stride;
    // the pairs; a slot past V weighs nothing and is later than every time
    unsigned long long t[E];
    uint32_t w[E];
#pragma unroll
    for (uint32_t u = 0; u < E; u++) {
        const uint32_t v = tid + u * T;
        t[u] = ~0ull;
        w[u] = 0;
        if (v < a.V) {
            unsigned long long mt;
            const uint32_t kind = merged_time(a, row, v, &mt);
            if (a.merged) a.merged[(uint64_t)i * a.V + v] = mt;
            t[u] = kind == 1 ? a.default_time : mt;
            w[u] = kind ? a.weights[v] : 0u;
        }
    }
    if (!a.median) return;
    // honest weight, the smallest time of all pairs, the range of the weighted ones
    uint32_t honest = 0;
    unsigned long long all = ~0ull, lo = ~0ull, hi = 0;
#pragma unroll
    for (uint32_t u = 0; u < E; u++) {
        honest += w[u];
        all = t[u] < all ? t[u] : all;
        if (w[u]) {
            lo = t[u] < lo ? t[u] : lo;
            hi = t[u] > hi ? t[u] : hi;
        }
    }
    honest = wave_sum(honest);
    all = wave_min(all);
    lo = wave_min(lo);
    hi = wave_max(hi);
    if (tid % 64 == 0) sHonest[wave] = honest, sAll[wave] = all, sLo[wave] = lo, sHi[wave] = hi;
    __syncthreads();
    honest = 0, all = ~0ull, lo = ~0ull, hi = 0;
    for (uint32_t k = 0; k < nw; k++) {
        honest += sHonest[k];
        all = sAll[k] < all ? sAll[k] : all;
        lo = sLo[k] < lo ? sLo[k] : lo;
        hi = sHi[k] > hi ? sHi[k] : hi;
    }
    // total weight < 2^31, so uint32 sums are exact
    const uint32_t half = honest / 2;
    unsigned long long ans;
    if (half == 0) {
        ans = all;
    } else if (lo == hi) {
        ans = lo;
    } else {
        // every weighted time lies in [lo, hi] and shares their common prefix;
        // below it: bit set iff the weight at or below (ans | lower bits) misses half.
        // Every value is the same in all threads, so the barriers are uniform
        const int top = 63 - __clzll((long long)(lo ^ hi));
        ans = hi & ~((2ull << top) - 1ull);
        for (int bit = top; bit >= 0; bit--) {
            const unsigned long long cand = ans | ((1ull << bit) - 1ull);
            uint32_t part = 0;
#pragma unroll
            for (uint32_t u = 0; u < E; u++) part += t[u] <= cand ? w[u] : 0u;
            part = wave_sum(part);
            // two buffers: a wave a whole round ahead has passed the barrier
            // every reader of this round's buffer arrives at only after reading
            uint32_t *buf = sW[bit & 1];
            if (tid % 64 == 0) buf[wave] = part;
            __syncthreads();
            uint32_t sum = 0;
            for (uint32_t k = 0; k < nw; k++) sum += buf[k];
            if (sum < half) ans |= 1ull << bit;
        }
    }
    if (tid == 0) a.median[i] = ans;
}

}  // namespace

hipError_t launch_mt(const MtArgs &a, hipStream_t s) {
    if (!a.n) return hipSuccess;
    if (!a.V || a.V > kMtMaxV) return hipErrorInvalidValue;
    const uint32_t E = (a.V + kMtThreads - 1) / kMtThreads;
    const dim3 grid(a.n), block(E == 1 ? (a.V + 63) / 64 * 64 : kMtThreads);
    if (E == 1) hipLaunchKernelGGL(k_mt<1>, grid, block, 0, s, a);
    else if (E == 2) hipLaunchKernelGGL(k_mt<2>, grid, block, 0, s, a);
    else if (E <= 4) hipLaunchKernelGGL(k_mt<4>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(k_mt<8>, grid, block, 0, s, a);
    return hipGetLastError();
}

}  // namespace lx
