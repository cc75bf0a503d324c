// lx_index_get.cpp -- the row getters of the index handle (lx_index.h) and the resident
// row server.
#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <cstring>

#include "lx_index.h"

using namespace lxi;

namespace {

// Rows of n events in the reference byte layout (mode 0 HighestBefore, 1
// LowestAfter, 2 merged HighestBefore), encoded on the device by k_get_rows
// straight into the pinned buffer: one launch and one stream sync per call
// (rows of more than kGetChunk bytes go in several).  *rows: row i at
// rows + i * slot; len[i] its byte length.
constexpr uint64_t kGetChunk = 64ull << 20;

// single-row tags: 30 bits (the server's request word), never 0 or kGetSrvStop
uint32_t next_get_tag(lx_index *h) {
    h->srv.get_tag = h->srv.get_tag + 1 >= kGetSrvStop ? 1u : h->srv.get_tag + 1;
    return h->srv.get_tag;
}

// the server's arguments for a single-row GetArgs (memcmp-comparable)
GetSrvArgs srv_args_of(const lx_index *h, const GetArgs &a) {
    GetSrvArgs s;
    memset(&s, 0, sizeof s);
    s.g = a;
    s.g.plane = nullptr;
    s.g.ev = nullptr;
    s.g.ev0 = 0;
    s.g.mode = 0;
    s.g.tag = 0;
    // a server outlives Adds: its bound is the handle's capacity (rows past
    // n_events are zero or stale there; the host check, option
    // getter_host_check, refuses such events before any request is posted),
    // so that an Add between two getters does not relaunch it
    if (!h->rowseg()) s.g.row_hi = (uint32_t)std::min<uint64_t>(h->n_cap, 0xFFFFFFFFull);
    s.hb = h->lay.hb;
    s.la = h->lay.la;
    s.req = h->srv.host.dev();
    s.exited = reinterpret_cast<uint32_t *>(h->srv.host.dev() + 1);
    return s;
}

// (re)launch the server with the arguments of `a`; it ignores request tags up
// to seen0
int srv_launch(lx_index *h, const GetArgs &a, uint32_t seen0) {
    GetSrvArgs s = srv_args_of(h, a);
    h->srv.args = s;
    s.gen = ++h->srv.gen;
    s.seen0 = seen0;
    s.idle_ticks = 250 * h->srv.ticks_us;          // leave after 250 us without a request
    s.budget_ticks = 500000 * h->srv.ticks_us;     // and after 0.5 s in all
    HIPCHK(h, lx::launch_get_server(s, h->srv.stream));
    h->srv.live = true;
    h->srv.launches++;
    return 0;
}

}  // namespace

// stop a live server (the stop tag, then its stream): it reads nothing but
// the request word between requests
void srv_stop(lx_index *h) {
    if (!h || !h->srv.live) return;
    static_cast<volatile uint64_t *>(h->srv.host.host())[0] = kGetSrvStop;
    (void)hipStreamSynchronize(h->srv.stream);
    h->srv.live = false;
}

namespace {

// post one row request to the server when the handle's stream is idle (every
// row the request reads is final); *posted = false: the caller launches
int srv_post(lx_index *h, const GetArgs &a, bool *posted) {
    *posted = false;
    if (!h->srv.opt || a.n != 1 || a.ev) return 0;
    if (h->srv.opt == 1 && lx_live_handles() > 1) {
        // another handle's streams may share the server's hardware queue
        if (h->srv.live) srv_stop(h);
        return 0;
    }
    // the rows it reads must be final: wait for the stream (usually the tail
    // of a launch whose results the host already has -- a pinned-path
    // ForklessCause, a getter that launched -- so that the next call finds it
    // idle instead of launching again)
    if (hipStreamQuery(h->stream) != hipSuccess && hipStreamSynchronize(h->stream) != hipSuccess) return 0;
    if (!h->srv.host.host()) {
        // what the server needs; without any of it the getters launch as before
        int lo = 0, hi = 0, khz = 0;
        bool ok = hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, h->device) == hipSuccess && khz >= 1000 &&
                  hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess;
        if (ok && !h->srv.stream) ok = hipStreamCreateWithPriority(&h->srv.stream.s, hipStreamNonBlocking, hi) == hipSuccess;
        if (ok) ok = h->srv.host.grow(8, 8, nullptr, false) == hipSuccess;
        if (!ok) {
            (void)hipGetLastError();
            h->srv.opt = 0;
            return 0;
        }
        memset(h->srv.host.host(), 0, 64);
        h->srv.ticks_us = (uint64_t)khz / 1000;
    }
    volatile uint64_t *req = h->srv.host.host();
    const GetSrvArgs want = srv_args_of(h, a);
    if (h->srv.live && (uint32_t)static_cast<volatile uint64_t *>(h->srv.host.host())[1] == h->srv.gen) {
        (void)hipStreamSynchronize(h->srv.stream);   // it left (idle or deadline): its launch has ended
        h->srv.live = false;
    }
    if (h->srv.live && memcmp(&want, &h->srv.args, sizeof want) != 0) srv_stop(h);
    int rc;
    if (!h->srv.live && (rc = srv_launch(h, a, (uint32_t)(req[0] & kGetSrvStop)))) return rc;
    req[0] = (uint64_t)a.ev0 << 32 | (uint64_t)(a.mode & 3u) << 30 | a.tag;
    *posted = true;
    return 0;
}

int get_rows(lx_index *h, uint32_t mode, uint32_t n, const uint32_t *ev, uint8_t **rows, uint64_t *slot,
             const uint32_t **len) {
    const uint64_t sl = ((uint64_t)8 * std::max(h->B, h->V) + 15) / 16 * 16;
    const uint64_t head = ((uint64_t)8 * n + 4 + 15) / 16 * 16;   // events + lengths + completion tag
    int rc;
    if ((rc = h->ensure_qp(head + n * sl))) return rc;
    uint8_t *const hp = h->qp.host(), *const dp = h->qp.dev();
    if (n > 1) memcpy(hp, ev, n * 4ull);
    GetArgs a{};
    a.plane = mode == 1 ? h->lay.la : h->lay.hb;
    a.stride = h->stride;
    // one row: the event travels in the arguments (no read of host memory)
    a.ev = n > 1 ? reinterpret_cast<const uint32_t *>(dp) : nullptr;
    a.ev0 = ev[0];
    a.n = n;
    a.B = h->B;
    a.V = h->V;
    a.mode = mode;
    a.forks = h->B > h->V ? 1u : 0u;
    a.ev_bbefore = h->lay.ev_bbefore;
    a.ev_branch = h->lay.ev_branch;
    a.branch_first = h->lay.branch_first;
    a.cheat_of = h->lay.cheat_of;
    a.cheat_off = h->lay.cheat_off;
    a.cheat_br = h->lay.cheat_br;
    a.len = reinterpret_cast<uint32_t *>(dp + 4ull * n);
    a.out = dp + head;
    a.slot = sl;
    // the device's own bound: the events indexed so far on a launch (the
    // resident server's bound is the capacity instead, srv_args_of)
    a.row_lo = h->rowseg() ? h->rs_lo : 0u;
    a.row_hi = h->rowseg() ? h->rs_hi : (uint32_t)h->n_events;
    if (n == 1) {
        // one row (the reference's per-call getters): the resident server
        // answers it when the handle's stream is idle (no launch); otherwise a
        // launch on the stream.  Either publishes a tag after the row and the
        // host spins on it (a stream synchronization costs ~5 us more,
        // scripts/probes/sync_latency.hip); a launch that never lands is caught
        // by the timeout's synchronization
        a.tag = next_get_tag(h);
        a.done = reinterpret_cast<uint32_t *>(dp + 8ull * n);
        const volatile uint32_t *done = reinterpret_cast<const volatile uint32_t *>(hp + 8ull * n);
        bool posted = false;
        if ((rc = srv_post(h, a, &posted))) return rc;
        if (!posted) {
            h->srv.fallbacks++;
            HIPCHK(h, lx::launch_get_rows(a, h->stream));
        }
        const auto t0 = std::chrono::steady_clock::now();
        bool relaunched = false;
        for (uint32_t k = 0; *done != a.tag; k++) {
            if ((k & 63) != 63) continue;
            if (posted && !relaunched &&
                (uint32_t)static_cast<volatile uint64_t *>(h->srv.host.host())[1] == h->srv.gen && *done != a.tag) {
                // the server left (idle or its deadline) before it saw the request
                h->srv.live = false;
                if ((rc = srv_launch(h, a, a.tag == 1 ? kGetSrvStop - 1 : a.tag - 1))) return rc;
                relaunched = true;
            }
            if ((k & 1023) == 1023 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(200)) {
                if (posted && *done != a.tag) {
                    // the server did not answer: stop it and take the launch path
                    srv_stop(h);
                    if (*done != a.tag) {
                        posted = false;
                        h->srv.fallbacks++;
                        HIPCHK(h, lx::launch_get_rows(a, h->stream));
                    }
                }
                HIPCHK(h, hipStreamSynchronize(h->stream));
                if (*done != a.tag) return h->fail(LX_ERR_STATE, "getter: the row kernel did not complete");
            }
        }
        if (posted) h->srv.served++;
        std::atomic_thread_fence(std::memory_order_acquire);
    } else {
        HIPCHK(h, lx::launch_get_rows(a, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    *rows = hp + head;
    *slot = sl;
    *len = reinterpret_cast<const uint32_t *>(hp + 4ull * n);
    for (uint32_t i = 0; i < n; i++)
        if ((*len)[i] == kGetBadLen) return h->fail(LX_ERR_ARG, "unknown event %u (refused by the row kernel)", ev[i]);
    return 0;
}

int get_check(lx_index *h, uint32_t n, const uint32_t *ev) {
    if (h->sharded())
        return h->fail(LX_ERR_STATE, "a column shard holds its own columns: lx_shard_get_rows (or lx_get_rows_dev + a sum over the shards)");
    if (!h->have_epoch) return h->fail(LX_ERR_STATE, "getter before lx_reset");
    NOT_LOADING(h);
    if (h->rowseg()) {
        // a row-segment rank answers for its own rows (final after lx_rowseg_finish);
        // the others' are routed to their owners (lachesis_hip/rowseg.py, lx_rowseg_get_rows)
        if (h->rs_state != 4) return h->fail(LX_ERR_STATE, "row-segment rank: getters before lx_rowseg_finish");
        if (h->get_host_check)
            for (uint32_t i = 0; i < n; i++)
                if (ev[i] < h->rs_lo || ev[i] >= h->rs_hi)
                    return h->fail(ev[i] < h->n_events ? LX_ERR_STATE : LX_ERR_ARG,
                                   "event %u is not a row of this row-segment rank [%u, %u)", ev[i], h->rs_lo, h->rs_hi);
    }
    {
        const int rc = flush_pending(h);
        if (rc) return rc;
    }
    if (h->get_host_check)
        for (uint32_t i = 0; i < n; i++)
            if (ev[i] >= h->n_events) return h->fail(LX_ERR_ARG, "unknown event %u", ev[i]);
    HIPCHK(h, set_dev(h->device));
    return 0;
}

int get_one(lx_index *h, uint32_t mode, uint32_t ev, uint8_t *out, uint32_t cap, uint32_t *len) {
    if (!h) return LX_ERR_ARG;
    int rc;
    if ((rc = get_check(h, 1, &ev))) return rc;
    uint8_t *rows;
    uint64_t slot;
    const uint32_t *ln;
    if ((rc = get_rows(h, mode, 1, &ev, &rows, &slot, &ln))) return rc;
    if (len) *len = ln[0];
    if (out && cap) memcpy(out, rows, std::min(cap, ln[0]));   // little-endian host
    return 0;
}

int get_batch(lx_index *h, uint32_t mode, uint32_t n, const uint32_t *ev, uint64_t *off, uint8_t *out, uint64_t cap) {
    if (!h || (n && (!ev || !off))) return LX_ERR_ARG;
    int rc;
    if ((rc = get_check(h, n, ev))) return rc;
    off[0] = 0;
    const uint64_t sl = ((uint64_t)8 * std::max(h->B, h->V) + 15) / 16 * 16;
    const uint32_t chunk = (uint32_t)std::max<uint64_t>(1, kGetChunk / sl);
    for (uint32_t i0 = 0; i0 < n; i0 += chunk) {
        const uint32_t m = std::min(chunk, n - i0);
        uint8_t *rows;
        uint64_t slot;
        const uint32_t *ln;
        if ((rc = get_rows(h, mode, m, ev + i0, &rows, &slot, &ln))) return rc;
        for (uint32_t i = 0; i < m; i++) {
            off[i0 + i + 1] = off[i0 + i] + ln[i];
            if (out && off[i0 + i + 1] <= cap) memcpy(out + off[i0 + i], rows + i * slot, ln[i]);
        }
    }
    if (out && off[n] > cap)
        return h->fail(LX_ERR_ARG, "getter buffer too small: %llu bytes needed", (unsigned long long)off[n]);
    return 0;
}

}  // namespace

extern "C" {

int lx_get_event_branch_id(lx_index *h, uint32_t ev, uint32_t *out) {
    if (!h || !out) return LX_ERR_ARG;
    NOT_LOADING(h);
    if (ev >= h->n_events) return h->fail(LX_ERR_ARG, "failed to read event's branch ID (unknown event %u)", ev);
    if (h->hm.ok) {
        *out = h->hm.branch[ev];
        return 0;
    }
    HIPCHK(h, set_dev(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(out, h->lay.ev_branch + ev, 4, hipMemcpyDeviceToHost));
    return 0;
}

int lx_get_server_stats(const lx_index *h, uint64_t out[3]) {
    if (!h || !out) return LX_ERR_ARG;
    out[0] = h->srv.served;
    out[1] = h->srv.launches;
    out[2] = h->srv.fallbacks;
    return 0;
}

int lx_get_highest_before(lx_index *h, uint32_t ev, uint8_t *out, uint32_t cap, uint32_t *len) {
    return get_one(h, 0, ev, out, cap, len);
}

int lx_get_lowest_after(lx_index *h, uint32_t ev, uint8_t *out, uint32_t cap, uint32_t *len) {
    return get_one(h, 1, ev, out, cap, len);
}

int lx_get_merged_highest_before(lx_index *h, uint32_t ev, uint8_t *out, uint32_t cap, uint32_t *len) {
    return get_one(h, 2, ev, out, cap, len);
}

int lx_get_highest_before_batch(lx_index *h, uint32_t n, const uint32_t *ev, uint64_t *off, uint8_t *out,
                                uint64_t cap) {
    return get_batch(h, 0, n, ev, off, out, cap);
}

int lx_get_lowest_after_batch(lx_index *h, uint32_t n, const uint32_t *ev, uint64_t *off, uint8_t *out, uint64_t cap) {
    return get_batch(h, 1, n, ev, off, out, cap);
}

int lx_get_merged_highest_before_batch(lx_index *h, uint32_t n, const uint32_t *ev, uint64_t *off, uint8_t *out,
                                       uint64_t cap) {
    return get_batch(h, 2, n, ev, off, out, cap);
}

int lx_row_bytes_max(const lx_index *h, uint64_t *bytes) {
    if (!h || !bytes) return LX_ERR_ARG;
    *bytes = 8ull * std::max(h->B, h->V);
    return 0;
}

int lx_get_rows_dev(lx_index *h, uint32_t mode, uint32_t n, const uint32_t *ev_dev, uint8_t *out_dev,
                    uint64_t slot_bytes, uint32_t *len_dev) {
    if (!h || mode > 2 || (n && (!ev_dev || !out_dev || !len_dev))) return LX_ERR_ARG;
    if (!h->have_epoch) return h->fail(LX_ERR_STATE, "getter before lx_reset");
    NOT_LOADING(h);
    if (h->rowseg() && h->rs_state != 4) return h->fail(LX_ERR_STATE, "row-segment rank: getters before lx_rowseg_finish");
    if (slot_bytes < 8ull * std::max(h->B, h->V) || slot_bytes % 8)
        return h->fail(LX_ERR_ARG, "row slot of %llu bytes < %llu", (unsigned long long)slot_bytes,
                       8ull * std::max(h->B, h->V));
    int rc;
    if ((rc = flush_pending(h))) return rc;
    HIPCHK(h, set_dev(h->device));
    if (!n) return 0;
    GetArgs a{};
    a.plane = mode == 1 ? h->lay.la : h->lay.hb;
    a.stride = h->pstride;
    a.ev = ev_dev;
    a.n = n;
    a.B = h->B;
    a.V = h->V;
    a.mode = mode;
    a.forks = h->B > h->V ? 1u : 0u;
    a.ev_bbefore = h->lay.ev_bbefore;
    a.ev_branch = h->lay.ev_branch;
    a.branch_first = h->lay.branch_first;
    a.cheat_of = h->lay.cheat_of;
    a.cheat_off = h->lay.cheat_off;
    a.cheat_br = h->lay.cheat_br;
    a.len = len_dev;
    a.out = out_dev;
    a.slot = slot_bytes;
    a.row_lo = h->rowseg() ? h->rs_lo : 0u;
    a.row_hi = h->rowseg() ? h->rs_hi : (uint32_t)h->n_events;
    if (h->sharded()) {
        // this shard's branches only, the rest of every slot zero: the shards'
        // slots sum word by word to the whole row (lx_shard_get_rows)
        a.cmap = h->lay.cmap;
        HIPCHK(h, hipMemsetAsync(out_dev, 0, (uint64_t)n * slot_bytes, h->stream));
    }
    HIPCHK(h, lx::launch_get_rows(a, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

int lx_get_branches_info(lx_index *h, uint32_t *last_seq, uint32_t *creator_idx, uint32_t cap, uint32_t *n_branches) {
    if (!h) return LX_ERR_ARG;
    NOT_LOADING(h);
    if (n_branches) *n_branches = h->B;
    if (!cap) return 0;
    HIPCHK(h, set_dev(h->device));
    int rc;
    if ((rc = hm_sync(h))) return rc;
    const std::vector<uint32_t> &len = h->hm.blen;
    for (uint32_t b = 0; b < h->B && b < cap; b++) {
        if (last_seq) last_seq[b] = len[b] ? h->h_branch_first[b] + len[b] - 1 : 0;
        if (creator_idx) creator_idx[b] = h->h_branch_creator[b];
    }
    return 0;
}

}  // extern "C"
