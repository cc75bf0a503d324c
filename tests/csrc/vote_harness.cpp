// vote_harness.cpp -- GPU test harness of the election's vote kernels
// (k_vote_init / k_vote_round1 / k_vote_round of lx_abft_kernels.hip) through
// the library's own launchers lx::launch_votes and lx::launch_votes_multi, on
// an observe relation given as per-slot bitmaps instead of a DAG: the
// reference's election tests use a fake relation the engine cannot take as
// events.  Test infrastructure only (tests/test_gpu_votes.py).
//
// Frames k = 0..G (frame F + k) with their root slots; election e = 0..E-1
// decides frame F + e and votes in frames k = e + 1 .. G (round k - e).  The
// vote tables come back concatenated: for e, for k = e + 1 .. G: [slots(k)][stride].
//   merged 0: every table by launch_votes, row stride `stride` (>= every
//     v_hi), per election the steps (v_lo, v_hi, slot_from, slot_to) in order,
//     each over k = e + 1 .. G (slot range clipped to the frame) -- the order
//     of vote_frame / widen_window;
//   merged 1: the tables of one round of all elections in one
//     launch_votes_multi, window [0, stride), as run_elections_ahead lays
//     them out.
// Every index is range-checked on the host first; nothing is launched on a
// malformed input.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "lx_internal.h"

namespace {

std::string g_err;

int fail(int rc, const std::string &m) {
    g_err = m;
    return rc;
}

template <class T>
struct Dev {
    T *p = nullptr;
    ~Dev() {
        if (p) (void)hipFree(p);
    }
    hipError_t put(const T *src, uint64_t n) {
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&p), std::max<uint64_t>(n, 1) * sizeof(T));
        if (e != hipSuccess || !n) return e;
        return src ? hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice) : hipSuccess;
    }
};

#define VH_HIP(x)                                                                  \
    do {                                                                           \
        hipError_t e_ = (x);                                                       \
        if (e_ != hipSuccess) return fail(-2, std::string(#x ": ") + hipGetErrorString(e_)); \
    } while (0)

}  // namespace

extern "C" const char *vh_last_error() { return g_err.c_str(); }

extern "C" int vh_run(uint32_t V, const uint32_t *w, uint32_t quorum, uint32_t G, uint32_t E, const uint32_t *slot_off,
                      const uint32_t *ev, const uint32_t *creator, const uint32_t *dup, const uint64_t *bm_off,
                      const uint32_t *bm, uint64_t bm_words, uint32_t stride, uint32_t n_steps, const uint32_t *steps,
                      uint32_t merged, uint32_t *votes_out, uint64_t votes_words, unsigned long long *dec_out,
                      uint32_t *err_out) {
    // ---- checks: nothing below may index out of what was given
    if (!V || !w || !G || !E || E > G || !slot_off || !ev || !creator || !dup || !bm_off || !bm || !steps || !n_steps ||
        !votes_out || !dec_out || !err_out)
        return fail(-1, "null or empty argument");
    if (!stride || stride > V || stride > kVoteNoRoot) return fail(-1, "stride must be in [1, V]");
    if (slot_off[0] != 0) return fail(-1, "slot_off[0] != 0");
    for (uint32_t k = 0; k <= G; k++)
        if (slot_off[k + 1] < slot_off[k] || slot_off[k + 1] - slot_off[k] >= kVoteNoRoot)
            return fail(-1, "bad slot_off");
    const uint32_t n_slots = slot_off[G + 1];
    uint64_t wsum = 0;
    for (uint32_t v = 0; v < V; v++) wsum += w[v];
    if (wsum > 0x7FFFFFFFull) return fail(-1, "total stake above 2^31 - 1");
    std::vector<uint32_t> bm_len(n_slots, 0), has_dup(G + 1, 0);
    for (uint32_t k = 0; k <= G; k++) {
        const uint32_t n = slot_off[k + 1] - slot_off[k], np = k ? slot_off[k] - slot_off[k - 1] : 0;
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t s = slot_off[k] + i;
            if (creator[s] >= V) return fail(-1, "slot creator out of range");
            if (dup[s] != LX_NONE) {
                // the chain ends: strictly decreasing, same creator
                if (dup[s] >= i || creator[slot_off[k] + dup[s]] != creator[s]) return fail(-1, "bad dup chain");
                has_dup[k] = 1;
            }
            bm_len[s] = np;
            if (bm_off[s] > bm_words || (np + 31) / 32 > bm_words - bm_off[s]) return fail(-1, "bitmap outside bm");
        }
    }
    uint32_t all_to = 0;
    for (uint32_t k = 1; k <= G; k++) all_to = std::max(all_to, slot_off[k + 1] - slot_off[k]);
    for (uint32_t i = 0; i < n_steps; i++) {
        const uint32_t *st = steps + 4 * i;
        if (st[0] >= st[1] || st[1] > stride || st[2] > st[3]) return fail(-1, "bad step");
        if (merged && (n_steps != 1 || st[0] != 0 || st[1] != stride || st[2] != 0 || st[3] < all_to))
            return fail(-1, "merged: one step, the whole window, every slot");
    }
    // tables
    std::vector<uint64_t> toff((uint64_t)E * (G + 1), ~0ull);
    uint64_t vtot = 0;
    for (uint32_t e = 0; e < E; e++)
        for (uint32_t k = e + 1; k <= G; k++) {
            toff[(uint64_t)e * (G + 1) + k] = vtot;
            vtot += (uint64_t)(slot_off[k + 1] - slot_off[k]) * stride;
        }
    if (vtot != votes_words) return fail(-1, "votes_words does not match the tables");

    // ---- upload
    Dev<uint32_t> d_w, d_ev, d_creator, d_dup, d_bm, d_len, d_votes, d_err;
    Dev<uint64_t> d_bm_off;
    Dev<unsigned long long> d_dec;
    Dev<VoteArgs> d_args;
    VH_HIP(d_w.put(w, V));
    VH_HIP(d_ev.put(ev, n_slots));
    VH_HIP(d_creator.put(creator, n_slots));
    VH_HIP(d_dup.put(dup, n_slots));
    VH_HIP(d_bm.put(bm, bm_words));
    VH_HIP(d_len.put(bm_len.data(), n_slots));
    VH_HIP(d_bm_off.put(bm_off, n_slots));
    VH_HIP(d_votes.put(nullptr, vtot));
    VH_HIP(d_dec.put(nullptr, (uint64_t)E * stride));
    VH_HIP(d_err.put(nullptr, E));
    VH_HIP(hipMemset(d_votes.p, 0, std::max<uint64_t>(vtot, 1) * 4));   // 0 = not voted
    VH_HIP(hipMemset(d_dec.p, 0xFF, (uint64_t)E * stride * 8));
    VH_HIP(hipMemset(d_err.p, 0, E * 4ull));

    auto table = [&](uint32_t e, uint32_t k, uint32_t v_lo, uint32_t v_hi, uint32_t from) {
        VoteArgs a{};
        a.V = stride;
        a.voter_ev = d_ev.p + slot_off[k] + from;
        a.bm_off = d_bm_off.p + slot_off[k] + from;
        a.bm_len = d_len.p + slot_off[k] + from;
        a.bm = d_bm.p;
        a.prev_creator = d_creator.p + slot_off[k - 1];
        a.prev_dup = d_dup.p + slot_off[k - 1];
        a.prev_votes = k == e + 1 ? nullptr : d_votes.p + toff[(uint64_t)e * (G + 1) + k - 1];
        a.prev_has_dup = has_dup[k - 1];
        a.v_lo = v_lo;
        a.v_hi = v_hi;
        a.wcreator = d_w.p;
        a.quorum = quorum;
        a.votes = d_votes.p + toff[(uint64_t)e * (G + 1) + k] + (uint64_t)from * stride;
        a.dec = d_dec.p + (uint64_t)e * stride;
        a.err = d_err.p + e;
        return a;
    };

    if (!merged) {
        for (uint32_t e = 0; e < E; e++)
            for (uint32_t i = 0; i < n_steps; i++) {
                const uint32_t *st = steps + 4 * i;
                for (uint32_t k = e + 1; k <= G; k++) {
                    const uint32_t n = slot_off[k + 1] - slot_off[k];
                    const uint32_t from = std::min(st[2], n), to = std::min(st[3], n);
                    if (from == to) continue;
                    VH_HIP(lx::launch_votes(table(e, k, st[0], st[1], from), to - from, k == e + 1, nullptr));
                }
            }
    } else {
        std::vector<std::vector<VoteArgs>> by_round(G);
        for (uint32_t e = 0; e < E; e++)
            for (uint32_t k = e + 1; k <= G; k++) {
                VoteArgs a = table(e, k, 0, stride, 0);
                a.n_voters = slot_off[k + 1] - slot_off[k];
                by_round[k - e - 1].push_back(a);
            }
        std::vector<VoteArgs> flat;
        std::vector<uint64_t> aoff(G + 1, 0);
        for (uint32_t r = 0; r < G; r++) {
            flat.insert(flat.end(), by_round[r].begin(), by_round[r].end());
            aoff[r + 1] = flat.size();
        }
        VH_HIP(d_args.put(flat.data(), flat.size()));
        for (uint32_t r = 0; r < G; r++) {
            uint32_t mx = 0;
            for (const VoteArgs &a : by_round[r]) mx = std::max(mx, a.n_voters);
            VH_HIP(lx::launch_votes_multi(d_args.p + aoff[r], (uint32_t)by_round[r].size(), mx, stride, r == 0, nullptr));
        }
    }
    VH_HIP(hipDeviceSynchronize());
    if (vtot) VH_HIP(hipMemcpy(votes_out, d_votes.p, vtot * 4, hipMemcpyDeviceToHost));
    VH_HIP(hipMemcpy(dec_out, d_dec.p, (uint64_t)E * stride * 8, hipMemcpyDeviceToHost));
    VH_HIP(hipMemcpy(err_out, d_err.p, E * 4ull, hipMemcpyDeviceToHost));
    return 0;
}
