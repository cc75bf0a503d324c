// lx_index_fc.cpp -- ForklessCause on the index handle (lx_index.h): the kernel arguments,
// the entry points, the early-exit counters, the column-shard early exit.
#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <cstring>

#include "lx_index.h"

using namespace lxi;

int lx_fc_args(lx_index *h, uint64_t n, const uint32_t *a, const uint32_t *b, uint8_t *out, uint32_t *partial,
               FcArgs *fa) {
    if (!h->have_epoch) return h->fail(LX_ERR_STATE, "ForklessCause before lx_reset");
    NOT_LOADING(h);
    if (h->rowseg() && h->rs_state != 4)
        return h->fail(LX_ERR_STATE, "row-segment rank: ForklessCause before lx_rowseg_finish");
    FcArgs f{};
    f.hb = h->lay.hb;
    f.la = h->lay.la;
    f.stride = h->pstride;
    f.n_events = h->rowseg() ? h->rs_hi : (uint32_t)h->n_events;
    f.ev_lo = h->rowseg() ? h->rs_lo : 0u;
    f.b_stamp = h->rowseg() ? h->lay.rs_stamp : nullptr;
    f.n_all = (uint32_t)h->n_events;
    f.la_recv = h->rowseg() ? h->lay.rs_rla : nullptr;
    f.b_slot = h->rowseg() ? h->lay.rs_lslot : nullptr;
    f.b_arrived = 2 * h->rs_gen + 1;
    f.n = n;
    f.qa = a;
    f.qb = b;
    f.out = out;
    f.partial = partial;
    if (h->sharded()) {
        f.wpad = h->lay.wloc;     // local columns: own originals first
        f.vlo4 = 0;
        f.vhi4 = (h->own_hi - h->own_lo + 3) / 4;
        f.cmap = h->lay.cmap;
    } else {
        f.wpad = h->lay.wpad;
        f.vlo4 = h->own_lo / 4;
        f.vhi4 = (h->own_hi + 3) / 4;
        f.cmap = nullptr;
    }
    f.cheat_brl = h->lay.cheat_brl;
    f.cheat_crl = h->lay.cheat_crl;
    f.fk_w = h->lay.fk_w;
    f.fk_c = h->lay.fk_c;
    f.fk_wch = h->lay.fk_wch;
    f.fk_hi4 = h->fk_hi4;
    f.quorum = h->quorum;
    f.ev_branch = h->lay.ev_branch;
    f.ev_creator = h->lay.ev_creator;
    f.n_cheat = h->n_cheat;
    f.cheat_off = h->lay.cheat_off;
    f.cheat_br = h->lay.cheat_br;
    f.cheat_creator = h->lay.cheat_creator;
    f.own_lo = h->own_lo;
    f.own_hi = h->own_hi;
    f.branch_creator = h->lay.branch_creator;
    f.status = h->status;
    // early exit (k_fc_early: fork-free whole rows of more than 512 columns --
    // launch_fc's 64-lane width, the gate matches what runs): rounds of the
    // first 128, 256, 512 columns and the rest, when the heaviest 512 columns
    // can reach the quorum alone (else no round before the last can decide)
    // Small launches (the FC cache's row fills, calcFrameIdx-sized batches) keep
    // whole rows: all of a row's loads in one round is the shortest latency,
    // and the caller waits for the launch (drop-in C5: 4 rounds cost ~1.4 us
    // per miss)
    if (!partial && !h->sharded() && h->B == h->V && h->fc_early && f.vhi4 - f.vlo4 > 128 && n >= kFcEarlyMinQueries) {
        const uint32_t L = h->fc_early_lanes;   // rounds of 4L, 8L, 16L columns
        uint64_t w128 = 0, w256 = 0, w512 = 0, wt = 0;
        for (uint32_t c = f.vlo4 * 4; c < h->V && c < f.vhi4 * 4; c++) {
            const uint32_t k = c - f.vlo4 * 4;
            wt += h->weights[c];
            if (k < 4 * L) w128 += h->weights[c];
            if (k < 8 * L) w256 += h->weights[c];
            if (k < 16 * L) w512 += h->weights[c];
        }
        if (w512 >= h->quorum && wt - w128 <= 0xFFFFFFFFull) {
            if (!h->d_fc_full) {
                // zeroed and synchronized before any launch can count into it,
                // whatever stream runs that launch
                DevBuf<unsigned long long> p;
                HIPCHK(h, p.renew(4));
                hipError_t e = hipMemsetAsync(p, 0, 32, h->stream);
                if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
                if (e != hipSuccess) return h->hip(e, "ForklessCause early-exit counters");
                h->d_fc_full = std::move(p);
            }
            f.early = 1;
            f.early_rest = (uint32_t)(wt - w128);
            f.early_rest2 = (uint32_t)(wt - w256);
            f.early_rest3 = (uint32_t)(wt - w512);
            f.early_lanes = L;
            f.early_full = h->d_fc_full;
        }
    }
    // the same in fork epochs (k_fc_fk_early, option fc_early_forks): whole
    // handles whose fork tables are valid (1..64 cheaters), more than 512
    // original columns before the straddling uint4 (t0 > 128: round 4 has
    // columns, as the gate above asks of fork-free rows) and every fork branch
    // within one uint4 per lane of round 1.  rest[r]: every validator whose
    // original column is unread after round r + 1, cheaters included
    if (!partial && !h->sharded() && !h->rowseg() && h->B > h->V && h->fc_early && h->fc_early_forks && f.fk_hi4 &&
        n >= kFcEarlyMinQueries && h->own_lo == 0 && h->own_hi == h->V) {
        const uint32_t t0 = h->V / 4;
        if (t0 > 128 && f.fk_hi4 >= t0 && f.fk_hi4 - t0 <= 32) {
            uint64_t w512 = 0, r1 = 0, r2 = 0, r3 = 0;
            for (uint32_t c = 0; c < 4 * t0; c++) {
                const uint64_t wc = h->weights[c];
                if (c < 512) w512 += wc;
                if (c >= 128) r1 += wc;
                if (c >= 256) r2 += wc;
                if (c >= 512) r3 += wc;
            }
            if (w512 >= h->quorum && r1 <= 0xFFFFFFFFull) {
                if (!h->d_fc_fke) {
                    // zeroed and synchronized before any launch can count into it (as d_fc_full)
                    DevBuf<unsigned long long> p;
                    HIPCHK(h, p.renew(4));
                    hipError_t e = hipMemsetAsync(p, 0, 32, h->stream);
                    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
                    if (e != hipSuccess) return h->hip(e, "ForklessCause fork early-exit counters");
                    h->d_fc_fke = std::move(p);
                }
                f.fke = 1;
                f.fke_rest[0] = (uint32_t)r1;
                f.fke_rest[1] = (uint32_t)r2;
                f.fke_rest[2] = (uint32_t)r3;
                f.fke_t0 = t0;
                f.fke_full = h->d_fc_fke;
            }
        }
    }
    h->fc_unchecked = true;   // a query it cannot answer flags status[1]; lx_sync reports it
    *fa = f;
    return 0;
}

namespace {

// flush_pending for a launch on stream s: a foreign stream is not ordered after
// the handle's, so it waits for the run to finish
int flush_before(lx_index *h, hipStream_t s) {
    if (!h->pend.n) return 0;
    int rc = flush_pending(h);
    if (rc) return rc;
    if (s != h->stream) HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

constexpr uint64_t kFcPinnedMax = 1u << 16;   // per-call queries: pinned, device-mapped host buffer

// the four words of an early-exit counter buffer (all zero when there is none), read and cleared
int take_early_counters(lx_index *h, unsigned long long *dev, uint64_t c[4]) {
    HIPCHK(h, set_dev(h->device));
    for (int i = 0; i < 4; i++) c[i] = 0;
    if (!dev) return 0;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(c, dev, 32, hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemsetAsync(dev, 0, 32, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

}  // namespace

extern "C" {

int lx_fc_early_rounds(lx_index *h, uint64_t out[4]) {
    if (!h || !out) return LX_ERR_ARG;
    uint64_t c[4];
    if (int rc = take_early_counters(h, h->d_fc_full, c)) return rc;
    out[0] = c[2];   // queries the kernel decided on the early path (device count)
    out[1] = c[0];   // of them read columns 128-255
    out[2] = c[1];   // ... 256-511
    out[3] = c[3];   // ... the rest of both rows
    return 0;
}

int lx_fc_early_fork_rounds(lx_index *h, uint64_t out[4]) {
    if (!h || !out) return LX_ERR_ARG;
    return take_early_counters(h, h->d_fc_fke, out);   // past round 1, past round 2, every query, past round 3
}

int lx_fc_early_counters(lx_index *h, uint64_t *queries, uint64_t *second_round, uint64_t *whole_rows) {
    if (!queries || !second_round || !whole_rows) return LX_ERR_ARG;
    uint64_t r[4];
    const int rc = lx_fc_early_rounds(h, r);
    if (rc) return rc;
    *queries = r[0];
    *second_round = r[1];
    *whole_rows = r[3];
    return 0;
}

int lx_forkless_cause_batch_dev(lx_index *h, uint64_t n, const uint32_t *a, const uint32_t *b, uint8_t *out,
                                void *stream) {
    if (!h) return LX_ERR_ARG;
    if (!n) return 0;
    FcArgs f;
    int rc = lx_fc_args(h, n, a, b, out, nullptr, &f);
    if (rc) return rc;
    hipStream_t s = h->stream_or(stream);
    if ((rc = flush_before(h, s))) return rc;
    HIPCHK(h, lx::launch_fc(f, h->ncols, h->B > h->V, s));
    return 0;
}

int lx_forkless_cause_partial_dev(lx_index *h, uint64_t n, const uint32_t *a, const uint32_t *b, uint32_t *partial,
                                  void *stream) {
    if (!h) return LX_ERR_ARG;
    if (!n) return 0;
    FcArgs f;
    int rc = lx_fc_args(h, n, a, b, nullptr, partial, &f);
    if (rc) return rc;
    hipStream_t s = h->stream_or(stream);
    if ((rc = flush_before(h, s))) return rc;
    HIPCHK(h, lx::launch_fc(f, h->ncols, h->B > h->V, s));
    return 0;
}

// ---- column-shard early exit
int lx_fc_shard_early(const lx_index *h, uint32_t *rest) {
    if (!h) return 0;
    if (rest) *rest = 0;
    // fork-free (no shard's partial carries a mark or exceeds its stake) and
    // shard 0 able to decide something alone
    if (!h->sharded() || !h->have_epoch || h->B != h->V || h->weights.size() != h->V) return 0;
    uint32_t lo, hi;
    shard_bounds(h, 0, &lo, &hi);
    uint64_t w0 = 0, wt = 0;
    for (uint32_t c = 0; c < h->V; c++) {
        wt += h->weights[c];
        if (c >= lo && c < hi) w0 += h->weights[c];
    }
    if (wt - w0 > 0xFFFFFFFFull) return 0;
    if (rest) *rest = (uint32_t)(wt - w0);
    return (w0 >= h->quorum || wt - w0 < h->quorum) ? 1 : 0;
}

int lx_fc_shard_decide_dev(lx_index *h, uint64_t n, const uint32_t *partial, uint64_t *mask, void *stream) {
    if (!h || (n && (!partial || !mask))) return LX_ERR_ARG;
    uint32_t rest = 0;
    if (!lx_fc_shard_early(h, &rest)) return h->fail(LX_ERR_STATE, "the column-shard early exit does not apply (lx_fc_shard_early)");
    if (h->shard_rank != 0) return h->fail(LX_ERR_STATE, "only shard 0 decides early (its creators are the heaviest)");
    hipStream_t s = h->stream_or(stream);
    const uint64_t W = (n + 63) / 64;
    HIPCHK(h, lx::launch_fcs_decide(partial, n, h->quorum, rest, reinterpret_cast<unsigned long long *>(mask),
                                    reinterpret_cast<unsigned long long *>(mask) + W, s));
    return 0;
}

int lx_fc_shard_undecided_dev(lx_index *h, uint64_t n, const uint64_t *mask, const uint32_t *a, const uint32_t *b,
                              const uint32_t *partial, uint32_t *idx, uint32_t *a_out, uint32_t *b_out, uint32_t *p_out,
                              uint64_t *m) {
    if (!h || !m || (n && (!mask || !a || !b || !idx || !a_out || !b_out || (partial && !p_out)))) return LX_ERR_ARG;
    if (!h->sharded()) return h->fail(LX_ERR_STATE, "the column-shard early exit needs a column-sharded handle");
    if (n > 0x7FFFFFFFull) return h->fail(LX_ERR_ARG, "too many queries in one call");
    *m = 0;
    if (!n) return 0;
    HIPCHK(h, set_dev(h->device));
    if (n > h->fcs.flag.cap()) {
        (void)hipStreamSynchronize(h->stream);
        h->fcs.flag.reset();   // (the capacity the check above reads: set last)
        HIPCHK(h, h->fcs.pos.renew(n));
        HIPCHK(h, lx::fcs_scan_bytes(n, &h->fcs.tmp_bytes));
        HIPCHK(h, h->fcs.tmp.renew(std::max<size_t>(h->fcs.tmp_bytes, 16)));
        HIPCHK(h, h->fcs.flag.renew(n));
    }
    HIPCHK(h, lx::launch_fcs_undecided(reinterpret_cast<const unsigned long long *>(mask), n, a, b, partial, h->fcs.flag,
                                       h->fcs.pos, h->fcs.tmp, h->fcs.tmp_bytes, idx, a_out, b_out, p_out, h->stream));
    uint32_t cnt = 0;
    HIPCHK(h, hipMemcpyAsync(&cnt, h->fcs.pos + (n - 1), 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    *m = cnt;
    return 0;
}

int lx_fc_shard_answer_dev(lx_index *h, uint64_t n, const uint64_t *mask, uint64_t m, const uint32_t *idx,
                           const uint32_t *sum, uint8_t *out, void *stream) {
    if (!h || (n && (!mask || !out)) || (m && (!idx || !sum)) || m > n) return LX_ERR_ARG;
    hipStream_t s = h->stream_or(stream);
    const uint64_t W = (n + 63) / 64;
    const auto *dec = reinterpret_cast<const unsigned long long *>(mask);
    HIPCHK(h, lx::launch_fcs_answer(dec, dec + W, n, m, idx, sum, h->quorum, out, s));
    return 0;
}

int lx_fc_combine_dev(lx_index *h, uint64_t n, const uint32_t *sum, uint8_t *out, void *stream) {
    if (!h) return LX_ERR_ARG;
    hipStream_t s = h->stream_or(stream);
    HIPCHK(h, lx::launch_fc_combine(sum, out, n, h->quorum, s));
    return 0;
}

int lx_forkless_cause_batch(lx_index *h, uint64_t n, const uint32_t *a, const uint32_t *b, uint8_t *out) {
    if (!h) return LX_ERR_ARG;
    if (!n) return 0;
    HIPCHK(h, set_dev(h->device));
    {
        const int rc = flush_pending(h);
        if (rc) return rc;
    }
    if (n <= kFcPinnedMax) {
        // per-call sizes (calcFrameIdx asks ~2/3 V pairs, the election |roots|):
        // the kernel reads the pairs from and writes the answers into pinned host
        // memory -- one launch and one stream sync, no copies
        int rc;
        if ((rc = h->ensure_qp(n * 9 + 16))) return rc;
        uint8_t *const hp = h->qp.host(), *const dp = h->qp.dev();
        memcpy(hp, a, n * 4);
        memcpy(hp + 4 * n, b, n * 4);
        FcArgs f;
        if ((rc = lx_fc_args(h, n, reinterpret_cast<uint32_t *>(dp), reinterpret_cast<uint32_t *>(dp + 4 * n), dp + 8 * n,
                          nullptr, &f)))
            return rc;
        f.status = h->status + 2;   // k_fc flags status[1] = word 3, the sink; unknown events answer 0xFF
        // completion by the answers themselves: each byte is written once
        // (0, 1 or 0xFF) over a 0xFE the host put there, so the host spins
        // until none is left instead of synchronizing the stream (~5 us)
        volatile uint8_t *ans = hp + 8 * n;
        memset(hp + 8 * n, 0xFE, n);
        HIPCHK(h, lx::launch_fc(f, h->ncols, h->B > h->V, h->stream));
        const auto t0 = std::chrono::steady_clock::now();
        for (uint64_t i = 0, k = 0; i < n; k++) {
            while (i < n && ans[i] != 0xFE) i++;
            if (i < n && (k & 1023) == 1023 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(200)) {
                HIPCHK(h, hipStreamSynchronize(h->stream));
                while (i < n && ans[i] != 0xFE) i++;
                if (i < n) return h->fail(LX_ERR_STATE, "ForklessCause: the kernel left answers unwritten");
            }
        }
        std::atomic_thread_fence(std::memory_order_acquire);
        memcpy(out, hp + 8 * n, n);
        for (uint64_t i = 0; i < n; i++)
            if (out[i] > 1) return h->fail(LX_ERR_ARG, "ForklessCause on an unknown event");   // forkless_cause.go:43-61
        return 0;
    }
    if (n > h->lay.q_a.cap()) {
        HIPCHK(h, renew_guarded(std::max<uint64_t>(n, 4096), h->lay.q_a, h->lay.q_b, h->lay.q_out));
    }
    HIPCHK(h, hipMemsetAsync(h->status + 1, 0, 4, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->lay.q_a, a, n * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->lay.q_b, b, n * 4, hipMemcpyHostToDevice, h->stream));
    int rc = lx_forkless_cause_batch_dev(h, n, h->lay.q_a, h->lay.q_b, h->lay.q_out, nullptr);
    if (rc) return rc;
    uint32_t bad = 0;
    HIPCHK(h, hipMemcpyAsync(out, h->lay.q_out, n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(&bad, h->status + 1, 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (bad) return h->fail(LX_ERR_ARG, "ForklessCause on an unknown event");   // forkless_cause.go:43-61 (crit)
    return 0;
}

}  // extern "C"
