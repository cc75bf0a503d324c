// lx_ancestry.cpp -- ancestry queries behind include/lachesis_ancestry.h.
//
// The handle owns one device table, a label per dense event; everything else
// a query reads (HighestBefore / LowestAfter planes, branch and seq of every
// event) is the index's own and is taken from its view at every call.  The
// table is keyed by dense index, so it follows the index's rollbacks as the
// MedianTime handle does (lx_mediantime.cpp): IndexView::epoch_gen / roll_gen
// say when indices were given to other events, lx_index_kept_since how many
// kept theirs.  The fork-evidence calls keep only the list of the last
// lx_anc_cheaters, which the same generations empty.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../include/lachesis_ancestry.h"
#include "lx_devbuf.h"
#include "lx_internal.h"

namespace {
constexpr uint64_t kAncPairChunk = 1ull << 22;   // pairs per launch
constexpr uint32_t kAncMaxB = kAncLdsBytes / 4;  // one row must fit the LDS budget
constexpr uint32_t kAncMaxPerWg = 4096;          // events per confirm workgroup, at most
constexpr uint64_t kAncForkChunk = 1ull << 20;   // (head, cheater) queries of one lx_anc_cheaters launch
}  // namespace

struct lx_anc {
    lx_index *ix = nullptr;
    std::string err;
    uint64_t epoch_gen = 0, roll_gen = 0;   // the index's rollbacks this handle has followed
    // labels[0, n_lab) are held (zero = none); an event at or above n_lab has none
    uint64_t n_lab = 0;
    uint64_t low = 0;                       // the lowest event without a label (<= n_lab)
    uint64_t last_n = 0;                    // events of the last confirm, in out_ev
    lxi::DevBuf<uint32_t> labels;
    lxi::DevBuf<uint32_t> d_head, d_x;      // a chunk of pairs
    lxi::DevBuf<uint8_t> d_obs;
    lxi::DevBuf<uint8_t> win;               // one confirm: AncArgs::win, cnt, off, the scan's scratch
    lxi::DevBuf<uint32_t> cnt, off;
    lxi::DevBuf<uint8_t> tmp;
    lxi::DevBuf<uint32_t> out_ev;
    lxi::DevBuf<uint32_t> res;              // [n_heads] n_new, then the low-water mark
    lxi::PinBuf<uint32_t> h_res;
    // fork evidence: the answers of a chunk of queries, and the list of the last lx_anc_cheaters
    uint64_t last_ch = 0;
    lxi::DevBuf<uint32_t> d_fx, d_fy, d_fs;
    lxi::DevBuf<uint32_t> ch_creator, ch_x, ch_y, ch_seq;

    int fail(int code, const char *fmt, ...) {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        err = buf;
        return code;
    }
    int hip(hipError_t e, const char *what) {
        if (e == hipSuccess) return 0;
        return fail(e == hipErrorOutOfMemory ? LX_ERR_NOMEM : LX_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
    }
};

#define AHIP(m, expr)                               \
    do {                                            \
        int _rc = (m)->hip((expr), #expr);          \
        if (_rc) return _rc;                        \
    } while (0)
#define ARC(expr)                                   \
    do {                                            \
        int _rc = (expr);                           \
        if (_rc) return _rc;                        \
    } while (0)

namespace {

// the index as it is now, and the handle brought up to it: a new epoch holds
// no labels, a rollback keeps those below the flushed count it left.  `flush`:
// the caller will read the events' rows (lx_index_view), else lx_index_peek
int follow(lx_anc *m, IndexView *iv, bool flush) {
    const int rc = flush ? lx_index_view(m->ix, iv) : lx_index_peek(m->ix, iv);
    if (rc) {
        m->err = lx_last_error(m->ix);
        return rc;
    }
    if (iv->shard_count > 1) return m->fail(LX_ERR_STATE, "ancestry needs an unsharded index");
    if (iv->epoch_gen != m->epoch_gen) {
        m->n_lab = m->low = m->last_n = m->last_ch = 0;
        m->epoch_gen = iv->epoch_gen;
    } else if (iv->roll_gen != m->roll_gen) {
        const uint64_t kept = lx_index_kept_since(m->ix, m->roll_gen);
        m->n_lab = std::min(m->n_lab, kept);
        m->low = std::min(m->low, kept);
        m->last_n = m->last_ch = 0;
    }
    m->roll_gen = iv->roll_gen;
    int cur = -1;   // (hipSetDevice costs microseconds: only when the device is not current)
    if (hipGetDevice(&cur) != hipSuccess || cur != iv->device) AHIP(m, hipSetDevice(iv->device));
    return 0;
}

// labels[0, need) held: the events the table did not reach carry none
int hold(lx_anc *m, uint64_t need, hipStream_t st) {
    if (need <= m->n_lab) return 0;
    if (need > m->labels.cap() || !m->labels.get())
        AHIP(m, m->labels.regrow(std::max<uint64_t>({need, 2 * m->labels.cap(), 4096}), m->n_lab, lxi::Fill::tail, st));
    else
        AHIP(m, hipMemsetAsync(m->labels + m->n_lab, 0, (need - m->n_lab) * 4, st));
    m->n_lab = need;
    return 0;
}

// the index's tables of a fork-evidence launch; LX_ERR_ARG where a creator has
// more branches than a wave keeps intervals
int fork_args(lx_anc *m, const IndexView &iv, AncForkArgs *a) {
    for (const auto &l : *iv.by_creator)
        if (l.size() > kAncForkMaxBr)
            return m->fail(LX_ERR_ARG, "fork evidence supports up to %u branches of one creator", kAncForkMaxBr);
    *a = AncForkArgs{};
    a->hb = iv.hb;
    a->la = iv.la;
    a->stride = iv.stride;
    a->ev_branch = iv.ev_branch;
    a->ev_seq = iv.ev_seq;
    a->brow = iv.brow;
    a->branch_first = iv.branch_first;
    a->branch_len = iv.branch_len;
    a->s_cap = iv.s_cap;
    a->cheat_of = iv.cheat_of;
    a->cheat_off = iv.cheat_off;
    a->cheat_br = iv.cheat_br;
    a->cheat_creator = iv.cheat_creator;
    a->n_cheat = iv.n_cheat;
    return 0;
}

}  // namespace

extern "C" {

int lx_anc_create(lx_index *index, lx_anc **out) {
    if (!index || !out) return LX_ERR_ARG;
    lx_anc *m = new lx_anc();
    m->ix = index;
    const int rc = lx_anc_reset(m);
    if (rc) {
        lx_anc_destroy(m);
        return rc;
    }
    *out = m;
    return 0;
}

void lx_anc_destroy(lx_anc *m) { delete m; }   // (every launch was waited for by the call that made it)

const char *lx_anc_last_error(const lx_anc *m) { return m ? m->err.c_str() : "null handle"; }

int lx_anc_reset(lx_anc *m) {
    if (!m) return LX_ERR_ARG;
    m->epoch_gen = ~0ull;   // no generation of the index: follow() takes the epoch over
    IndexView iv;
    return follow(m, &iv, false);
}

int lx_anc_observes(lx_anc *m, uint64_t n, const uint32_t *head, const uint32_t *x, uint8_t *out) {
    if (!m) return LX_ERR_ARG;
    if (n && (!head || !x || !out)) return m->fail(LX_ERR_ARG, "null argument");
    if (!n) return 0;
    IndexView iv;
    ARC(follow(m, &iv, true));
    if (iv.loading) return m->fail(LX_ERR_STATE, "index is loading (lx_load_finish first)");
    for (uint64_t i = 0; i < n; i++) {
        if (head[i] >= iv.n_events) return m->fail(LX_ERR_ARG, "unknown event %u (head)", head[i]);
        if (x[i] >= iv.n_events) return m->fail(LX_ERR_ARG, "unknown event %u", x[i]);
    }
    AncPairArgs a{};
    a.hb = iv.hb;
    a.la = iv.la;
    a.stride = iv.stride;
    a.ev_branch = iv.ev_branch;
    a.ev_seq = iv.ev_seq;
    const uint64_t chunk = std::min(n, kAncPairChunk);
    // (every launch that read the old buffers has been waited for below)
    AHIP(m, m->d_head.grow(chunk));
    AHIP(m, m->d_x.grow(chunk));
    AHIP(m, m->d_obs.grow(chunk));
    a.head = m->d_head;
    a.x = m->d_x;
    a.out = m->d_obs;
    for (uint64_t lo = 0; lo < n; lo += chunk) {
        a.n = std::min(chunk, n - lo);
        AHIP(m, hipMemcpyAsync(m->d_head, head + lo, a.n * 4, hipMemcpyHostToDevice, iv.stream));
        AHIP(m, hipMemcpyAsync(m->d_x, x + lo, a.n * 4, hipMemcpyHostToDevice, iv.stream));
        AHIP(m, lx::launch_anc_pairs(a, iv.stream));
        AHIP(m, hipMemcpyAsync(out + lo, m->d_obs, a.n, hipMemcpyDeviceToHost, iv.stream));
        AHIP(m, hipStreamSynchronize(iv.stream));
    }
    return 0;
}

int lx_anc_confirm(lx_anc *m, uint32_t n_heads, const uint32_t *head, const uint32_t *label, uint32_t *n_new) {
    if (!m) return LX_ERR_ARG;
    if (n_heads && (!head || !label || !n_new)) return m->fail(LX_ERR_ARG, "null argument");
    IndexView iv;
    ARC(follow(m, &iv, true));
    if (iv.loading) return m->fail(LX_ERR_STATE, "index is loading (lx_load_finish first)");
    uint32_t top = 0;
    for (uint32_t k = 0; k < n_heads; k++) {
        if (head[k] >= iv.n_events) return m->fail(LX_ERR_ARG, "unknown event %u (head %u)", head[k], k);
        if (!label[k]) return m->fail(LX_ERR_ARG, "label 0 (head %u): 0 means no label", k);
        top = std::max(top, head[k]);
    }
    if (iv.B > kAncMaxB) return m->fail(LX_ERR_ARG, "lx_anc_confirm supports up to %u branches", kAncMaxB);
    m->last_n = 0;
    if (!n_heads) return 0;
    memset(n_new, 0, n_heads * 4ull);
    ARC(hold(m, (uint64_t)top + 1, iv.stream));
    // every event below `low` has a label; the table ends at n_lab
    const uint32_t lo = (uint32_t)m->low, hi = (uint32_t)m->n_lab;
    if (lo >= hi) return 0;   // (low > top: nothing left to label)
    const uint32_t range = hi - lo;
    const bool vec = iv.stride % 4 == 0;
    AncArgs a{};
    a.hb = iv.hb;
    a.la = iv.la;
    a.stride = iv.stride;
    a.B = iv.B;
    a.row_words = vec ? (iv.B + 3) & ~3u : iv.B;
    a.ev_branch = iv.ev_branch;
    a.ev_seq = iv.ev_seq;
    a.labels = m->labels;
    a.lo = lo;
    a.hi = hi;
    const uint32_t H = std::max(1u, std::min(kAncMaxHeads, kAncLdsBytes / (4 * a.row_words)));
    // a workgroup stages the rows once: enough events to stream about as many bytes (12 B each)
    const uint64_t stage = (uint64_t)std::min(H, n_heads) * a.row_words * 4;
    a.per_wg = (uint32_t)std::min<uint64_t>(kAncMaxPerWg, (stage / 16 + kAncThreads - 1) / kAncThreads * kAncThreads);
    a.per_wg = std::max(a.per_wg, kAncThreads);
    a.n_wg = (uint32_t)(((uint64_t)range + a.per_wg - 1) / a.per_wg);
    const uint64_t n_cnt = 2 + (uint64_t)kAncMaxHeads * a.n_wg;
    if (n_cnt > 0x7FFFFFFFull) return m->fail(LX_ERR_ARG, "too many events for one confirm");
    size_t tmp_bytes = 0;
    AHIP(m, lx::anc_scan_bytes((uint32_t)n_cnt, &tmp_bytes));
    // (every launch that read the old buffers was waited for by the call that made it)
    AHIP(m, m->win.grow(range));
    AHIP(m, m->out_ev.grow(range));
    AHIP(m, m->cnt.grow(n_cnt));
    AHIP(m, m->off.grow(n_cnt));
    AHIP(m, m->tmp.grow(std::max<size_t>(tmp_bytes, 1)));
    AHIP(m, m->res.grow((uint64_t)n_heads + 1));
    AHIP(m, m->h_res.grow((uint64_t)n_heads + 1));
    a.win = m->win;
    a.cnt = m->cnt;
    a.off = m->off;
    a.out_ev = m->out_ev;
    a.out_cap = range;
    a.low = m->res + n_heads;
    AHIP(m, hipMemsetAsync(m->cnt, 0, 4, iv.stream));
    for (uint32_t k0 = 0; k0 < n_heads; k0 += H) {
        a.H = std::min(H, n_heads - k0);
        a.top = 0;
        for (uint32_t k = 0; k < a.H; k++) {
            a.head[k] = head[k0 + k];
            a.label[k] = label[k0 + k];
            a.top = std::max(a.top, a.head[k]);
        }
        a.n_new = m->res + k0;
        // the mark is what the last launch leaves: it sees every label of the call
        AHIP(m, hipMemsetAsync(a.low, 0xFF, 4, iv.stream));
        AHIP(m, lx::launch_anc_confirm(a, m->tmp, tmp_bytes, iv.stream));
    }
    // counts and the mark in one read
    AHIP(m, hipMemcpyAsync(m->h_res, m->res, ((uint64_t)n_heads + 1) * 4, hipMemcpyDeviceToHost, iv.stream));
    AHIP(m, hipStreamSynchronize(iv.stream));
    uint64_t total = 0;
    for (uint32_t k = 0; k < n_heads; k++) total += n_new[k] = m->h_res[k];
    m->last_n = total;
    m->low = m->h_res[n_heads] == LX_NONE ? hi : m->h_res[n_heads];
    return 0;
}

int lx_anc_last_confirmed(lx_anc *m, uint32_t *out_ev, uint64_t cap, uint64_t *n) {
    if (!m) return LX_ERR_ARG;
    if (!n || (cap && !out_ev)) return m->fail(LX_ERR_ARG, "null argument");
    IndexView iv;
    ARC(follow(m, &iv, false));
    *n = m->last_n;
    const uint64_t c = std::min(cap, m->last_n);
    if (c) {
        AHIP(m, hipMemcpyAsync(out_ev, m->out_ev, c * 4, hipMemcpyDeviceToHost, iv.stream));
        AHIP(m, hipStreamSynchronize(iv.stream));
    }
    return 0;
}

int lx_anc_fork_pairs(lx_anc *m, uint64_t n, const uint32_t *head, const uint32_t *creator, uint32_t *out_x,
                      uint32_t *out_y, uint32_t *out_seq) {
    if (!m) return LX_ERR_ARG;
    if (n && (!head || !creator || !out_x || !out_y)) return m->fail(LX_ERR_ARG, "null argument");
    if (!n) return 0;
    IndexView iv;
    ARC(follow(m, &iv, true));
    if (iv.loading) return m->fail(LX_ERR_STATE, "index is loading (lx_load_finish first)");
    for (uint64_t i = 0; i < n; i++) {
        if (head[i] >= iv.n_events) return m->fail(LX_ERR_ARG, "unknown event %u (head)", head[i]);
        if (creator[i] >= iv.V) return m->fail(LX_ERR_ARG, "unknown creator %u: %u validators", creator[i], iv.V);
    }
    if (iv.B == iv.V || !iv.n_cheat) {   // no forks this epoch
        memset(out_x, 0xFF, n * 4);
        memset(out_y, 0xFF, n * 4);
        if (out_seq) memset(out_seq, 0, n * 4);
        return 0;
    }
    AncForkArgs a;
    ARC(fork_args(m, iv, &a));
    const uint64_t chunk = std::min(n, kAncPairChunk);
    // (every launch that read the old buffers has been waited for below)
    AHIP(m, m->d_head.grow(chunk));
    AHIP(m, m->d_x.grow(chunk));
    AHIP(m, m->d_fx.grow(chunk));
    AHIP(m, m->d_fy.grow(chunk));
    AHIP(m, m->d_fs.grow(chunk));
    a.head = m->d_head;
    a.creator = m->d_x;
    a.x = m->d_fx;
    a.y = m->d_fy;
    a.seq = m->d_fs;
    for (uint64_t lo = 0; lo < n; lo += chunk) {
        a.n = std::min(chunk, n - lo);
        AHIP(m, hipMemcpyAsync(m->d_head, head + lo, a.n * 4, hipMemcpyHostToDevice, iv.stream));
        AHIP(m, hipMemcpyAsync(m->d_x, creator + lo, a.n * 4, hipMemcpyHostToDevice, iv.stream));
        AHIP(m, lx::launch_anc_fork(a, iv.stream));
        AHIP(m, hipMemcpyAsync(out_x + lo, m->d_fx, a.n * 4, hipMemcpyDeviceToHost, iv.stream));
        AHIP(m, hipMemcpyAsync(out_y + lo, m->d_fy, a.n * 4, hipMemcpyDeviceToHost, iv.stream));
        if (out_seq) AHIP(m, hipMemcpyAsync(out_seq + lo, m->d_fs, a.n * 4, hipMemcpyDeviceToHost, iv.stream));
        AHIP(m, hipStreamSynchronize(iv.stream));
    }
    return 0;
}

int lx_anc_cheaters(lx_anc *m, uint32_t n_heads, const uint32_t *head, uint32_t *n_found) {
    if (!m) return LX_ERR_ARG;
    if (n_heads && (!head || !n_found)) return m->fail(LX_ERR_ARG, "null argument");
    IndexView iv;
    ARC(follow(m, &iv, true));
    if (iv.loading) return m->fail(LX_ERR_STATE, "index is loading (lx_load_finish first)");
    for (uint32_t k = 0; k < n_heads; k++)
        if (head[k] >= iv.n_events) return m->fail(LX_ERR_ARG, "unknown event %u (head %u)", head[k], k);
    AncForkArgs a{};
    const bool forks = iv.B != iv.V && iv.n_cheat;
    if (forks) ARC(fork_args(m, iv, &a));
    m->last_ch = 0;
    if (!n_heads) return 0;
    memset(n_found, 0, n_heads * 4ull);
    if (!forks) return 0;
    // launches of whole heads, at most kAncForkChunk queries each (one head at least)
    const uint32_t H = (uint32_t)std::min<uint64_t>(n_heads, std::max<uint64_t>(1, kAncForkChunk / iv.n_cheat));
    const uint64_t nq = (uint64_t)H * iv.n_cheat;
    if (nq + 1 > 0x7FFFFFFFull) return m->fail(LX_ERR_ARG, "too many cheaters for one launch");
    size_t tmp_bytes = 0;
    AHIP(m, lx::anc_scan_bytes((uint32_t)(nq + 1), &tmp_bytes));
    // (every launch that read the old buffers was waited for by the call that made it)
    AHIP(m, m->d_head.grow(H));
    AHIP(m, m->d_fx.grow(nq));
    AHIP(m, m->d_fy.grow(nq));
    AHIP(m, m->d_fs.grow(nq));
    AHIP(m, m->cnt.grow(nq + 1));
    AHIP(m, m->off.grow(nq + 1));
    AHIP(m, m->tmp.grow(std::max<size_t>(tmp_bytes, 1)));
    AHIP(m, m->res.grow(H));
    a.head = m->d_head;
    a.creator = nullptr;
    a.x = m->d_fx;
    a.y = m->d_fy;
    a.seq = m->d_fs;
    AncForkListArgs l{};
    l.x = a.x;
    l.y = a.y;
    l.seq = a.seq;
    l.cheat_creator = iv.cheat_creator;
    l.n_cheat = iv.n_cheat;
    l.flag = m->cnt;
    l.off = m->off;
    l.n_found = m->res;
    uint64_t total = 0;
    for (uint32_t k0 = 0; k0 < n_heads; k0 += H) {
        l.n_heads = std::min(H, n_heads - k0);
        a.n = (uint64_t)l.n_heads * iv.n_cheat;
        // the list holds what the earlier launches found and has room for every query of this one
        const uint64_t need = total + a.n;
        if (need > m->ch_x.cap() || !m->ch_x.get()) {
            const uint64_t cap = std::max<uint64_t>({need, 2 * m->ch_x.cap(), 1024});
            for (auto *b : {&m->ch_creator, &m->ch_x, &m->ch_y, &m->ch_seq})
                AHIP(m, b->regrow(cap, total, lxi::Fill::none, iv.stream));
        }
        l.base = total;
        l.out_creator = m->ch_creator;
        l.out_x = m->ch_x;
        l.out_y = m->ch_y;
        l.out_seq = m->ch_seq;
        AHIP(m, hipMemcpyAsync(m->d_head, head + k0, l.n_heads * 4ull, hipMemcpyHostToDevice, iv.stream));
        AHIP(m, lx::launch_anc_fork(a, iv.stream));
        AHIP(m, lx::launch_anc_fork_list(l, m->tmp, tmp_bytes, iv.stream));
        AHIP(m, hipMemcpyAsync(n_found + k0, m->res, l.n_heads * 4ull, hipMemcpyDeviceToHost, iv.stream));
        AHIP(m, hipStreamSynchronize(iv.stream));
        for (uint32_t k = 0; k < l.n_heads; k++) total += n_found[k0 + k];
    }
    m->last_ch = total;
    return 0;
}

int lx_anc_last_cheaters(lx_anc *m, uint32_t *out_creator, uint32_t *out_x, uint32_t *out_y, uint32_t *out_seq,
                         uint64_t cap, uint64_t *n) {
    if (!m) return LX_ERR_ARG;
    if (!n || (cap && (!out_creator || !out_x || !out_y))) return m->fail(LX_ERR_ARG, "null argument");
    IndexView iv;
    ARC(follow(m, &iv, false));
    *n = m->last_ch;
    const uint64_t c = std::min(cap, m->last_ch);
    if (c) {
        AHIP(m, hipMemcpyAsync(out_creator, m->ch_creator, c * 4, hipMemcpyDeviceToHost, iv.stream));
        AHIP(m, hipMemcpyAsync(out_x, m->ch_x, c * 4, hipMemcpyDeviceToHost, iv.stream));
        AHIP(m, hipMemcpyAsync(out_y, m->ch_y, c * 4, hipMemcpyDeviceToHost, iv.stream));
        if (out_seq) AHIP(m, hipMemcpyAsync(out_seq, m->ch_seq, c * 4, hipMemcpyDeviceToHost, iv.stream));
        AHIP(m, hipStreamSynchronize(iv.stream));
    }
    return 0;
}

int lx_anc_labels(lx_anc *m, uint64_t first, uint64_t n, uint32_t *out) {
    if (!m) return LX_ERR_ARG;
    if (n && !out) return m->fail(LX_ERR_ARG, "null argument");
    IndexView iv;
    ARC(follow(m, &iv, false));
    if (first + n < first || first + n > iv.n_events)
        return m->fail(LX_ERR_ARG, "events %llu..%llu: the index holds %llu", (unsigned long long)first,
                       (unsigned long long)(first + n), (unsigned long long)iv.n_events);
    if (!n) return 0;
    const uint64_t held = first < m->n_lab ? std::min(n, m->n_lab - first) : 0;
    if (held) {
        AHIP(m, hipMemcpyAsync(out, m->labels + first, held * 4, hipMemcpyDeviceToHost, iv.stream));
        AHIP(m, hipStreamSynchronize(iv.stream));
    }
    memset(out + held, 0, (n - held) * 4);
    return 0;
}

int lx_anc_set_labels(lx_anc *m, uint64_t first, uint64_t n, const uint32_t *labels) {
    if (!m) return LX_ERR_ARG;
    if (n && !labels) return m->fail(LX_ERR_ARG, "null argument");
    IndexView iv;
    ARC(follow(m, &iv, false));
    if (iv.loading) return m->fail(LX_ERR_STATE, "index is loading (lx_load_finish first)");
    if (first + n < first || first + n > iv.n_events)
        return m->fail(LX_ERR_ARG, "events %llu..%llu: the index holds %llu", (unsigned long long)first,
                       (unsigned long long)(first + n), (unsigned long long)iv.n_events);
    if (!n) return 0;
    ARC(hold(m, first + n, iv.stream));
    // queries run on the same stream; the caller's buffer is free on return
    AHIP(m, hipMemcpyAsync(m->labels + first, labels, n * 4, hipMemcpyHostToDevice, iv.stream));
    // the mark again, from the lower of the old one and the range
    const uint32_t lo = (uint32_t)std::min(m->low, first), hi = (uint32_t)m->n_lab;
    AHIP(m, m->res.grow(1));
    AHIP(m, m->h_res.grow(1));
    AHIP(m, hipMemsetAsync(m->res, 0xFF, 4, iv.stream));
    AHIP(m, lx::launch_anc_low(m->labels, lo, hi, m->res, iv.stream));
    AHIP(m, hipMemcpyAsync(m->h_res, m->res, 4, hipMemcpyDeviceToHost, iv.stream));
    AHIP(m, hipStreamSynchronize(iv.stream));
    m->low = m->h_res[0] == LX_NONE ? hi : m->h_res[0];
    return 0;
}

int lx_anc_low_water(lx_anc *m, uint64_t *ev) {
    if (!m) return LX_ERR_ARG;
    if (!ev) return m->fail(LX_ERR_ARG, "null argument");
    IndexView iv;
    ARC(follow(m, &iv, false));
    // (everything at or above n_lab is without a label, so low == n_lab names the next event)
    *ev = std::min<uint64_t>(m->low, iv.n_events);
    return 0;
}

}  // extern "C"
