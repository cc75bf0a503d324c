// lx_abft_build.hip -- the virtual HighestBefore rows of lx_abft_build_frames
// (DESIGN.md section 9c).
//
//   k_build_rows : one workgroup per candidate event that is NOT added.  Its row
//                  is what fillEventVectors (vecengine/index.go:144-209) would
//                  store: the join of its parents' rows (seq = max, the fork
//                  marker absorbing, vecfc/vector_ops.go:49-79), the own entry
//                  {seq, seq} on the branch it extends, and in a fork epoch the
//                  two fork-detection rules of :173-209 per cheater: (i) one
//                  marked branch marks all of the creator's branches, (ii) two
//                  non-empty branches whose [first seq, seq] intervals overlap
//                  mark all of them (MinSeq of a branch is its first seq).
//                  Rows go to a scratch plane with the index's row stride; the
//                  OWN forms of k_root_fc / k_root_fc16 (lx_abft_kernels.hip)
//                  read them in place of hb + ev * stride.
//
// Latency-bound: n workgroups, every thread streams its columns of the parent
// rows (coalesced, uint4 when the stride is a multiple of 4) and keeps the
// running join in registers; nothing is staged in LDS.  The cheater pass reads
// the finished row back from L2 (a few entries per cheater).
#include "lx_internal.h"

namespace lx {

template <bool FORKS, bool VEC>
__global__ __launch_bounds__(256) void k_build_rows(BuildRowsArgs a) {
    constexpr uint32_t W = VEC ? 4 : 1;
    const uint32_t c = blockIdx.x;
    if (c >= a.n) return;
    const uint32_t p0 = a.c.par_off[c], p1 = a.c.par_off[c + 1];
    const uint32_t be = a.c.br[c], sq = a.c.seq[c];
    uint32_t *row = a.plane + (uint64_t)c * a.stride;
    for (uint64_t j0 = (uint64_t)threadIdx.x * W; j0 < a.stride; j0 += 256 * W) {
        uint32_t s[W], m[W];
#pragma unroll
        for (uint32_t q = 0; q < W; q++) s[q] = m[q] = 0;
        if (j0 < a.B) {
#pragma unroll 4
            for (uint32_t p = p0; p < p1; p++) {
                const uint32_t *src = a.hb + (uint64_t)a.c.par[p] * a.stride + j0;
                uint32_t x[W];
                if (VEC) {
                    const uint4 v = *reinterpret_cast<const uint4 *>(src);
                    x[0] = v.x;
                    x[W > 1 ? 1 : 0] = v.y;
                    x[W > 2 ? 2 : 0] = v.z;
                    x[W > 3 ? 3 : 0] = v.w;
                } else {
                    x[0] = *src;
                }
#pragma unroll
                for (uint32_t q = 0; q < W; q++) {
                    m[q] |= x[q] & LX_MARK;
                    const uint32_t v = x[q] & LX_SEQ_MASK;
                    s[q] = v > s[q] ? v : s[q];
                }
            }
        }
        uint32_t o[W];
#pragma unroll
        for (uint32_t q = 0; q < W; q++) {
            const uint64_t j = j0 + q;
            if (j == be) s[q] = sq;   // the parents' entries of its own branch are below seq
            o[q] = j < a.B ? (s[q] | m[q]) : 0u;
        }
        if (VEC) {
            uint4 v;
            v.x = o[0];
            v.y = o[W > 1 ? 1 : 0];
            v.z = o[W > 2 ? 2 : 0];
            v.w = o[W > 3 ? 3 : 0];
            *reinterpret_cast<uint4 *>(row + j0) = v;
        } else {
            row[j0] = o[0];
        }
    }
    if (!FORKS) return;
    __syncthreads();   // the row is complete (global stores of this workgroup are visible to it)
    for (uint32_t i = threadIdx.x; i < a.n_cheat; i += 256) {
        const uint32_t *lst = a.c.cheat_br + a.c.cheat_off[i];
        const uint32_t m = a.c.cheat_off[i + 1] - a.c.cheat_off[i];
        bool hit = false;
        for (uint32_t x = 0; x < m && !hit; x++) {
            const uint32_t bx = lst[x], vx = row[bx], sx = vx & LX_SEQ_MASK;
            if (vx & LX_MARK) { hit = true; break; }
            if (!sx) continue;
            const uint32_t fx = a.branch_first[bx];   // a cheater's branches all hold events
            for (uint32_t y = x + 1; y < m; y++) {
                const uint32_t by = lst[y], vy = row[by], sy = vy & LX_SEQ_MASK;
                if (vy & LX_MARK) { hit = true; break; }
                if (!sy) continue;
                const uint32_t fy = a.branch_first[by];
                if (fx <= sy && fy <= sx) { hit = true; break; }
            }
        }
        if (hit)
            for (uint32_t x = 0; x < m; x++) row[lst[x]] |= LX_MARK;
    }
}

hipError_t launch_build_rows(const BuildRowsArgs &a, bool forks, hipStream_t s) {
    if (!a.n) return hipSuccess;
    const bool vec = a.stride % 4 == 0;
    if (forks && vec) hipLaunchKernelGGL((k_build_rows<true, true>), dim3(a.n), dim3(256), 0, s, a);
    else if (forks) hipLaunchKernelGGL((k_build_rows<true, false>), dim3(a.n), dim3(256), 0, s, a);
    else if (vec) hipLaunchKernelGGL((k_build_rows<false, true>), dim3(a.n), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((k_build_rows<false, false>), dim3(a.n), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace lx
