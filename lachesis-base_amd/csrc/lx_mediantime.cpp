// lx_mediantime.cpp -- MedianTime behind include/lachesis_mediantime.h.
//
// The handle owns one device table, the creation time of every dense event
// the caller handed over; everything else a query reads (HighestBefore plane,
// branch rows, the cheaters' branch lists, weights) is the index's own and is
// taken from its view at every call.  The table is keyed by dense index, so
// it follows the index's rollbacks: IndexView::epoch_gen / roll_gen say when
// indices were given to other events and lx_index_kept_since how many kept
// theirs (lx_index.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../include/lachesis_mediantime.h"
#include "lx_devbuf.h"
#include "lx_internal.h"

namespace {
constexpr uint32_t kMtChunk = 1u << 16;          // events per launch
constexpr uint64_t kMtRowBytes = 32ull << 20;    // merged rows per launch (device scratch)
}  // namespace

struct lx_mt {
    lx_index *ix = nullptr;
    std::string err;
    uint32_t V = 0;
    uint64_t epoch_gen = 0, roll_gen = 0;   // the index's rollbacks this handle has followed
    uint64_t n_times = 0;
    lxi::DevBuf<unsigned long long> times;  // [dense event]
    lxi::DevBuf<uint32_t> d_ev;             // a query's events (more than kMtInline)
    lxi::DevBuf<unsigned long long> d_rows; // merged rows of one launch
    lxi::MappedBuf<unsigned long long> med;   // medians of one launch, written by the kernel

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

#define MHIP(m, expr)                               \
    do {                                            \
        int _rc = (m)->hip((expr), #expr);          \
        if (_rc) return _rc;                        \
    } while (0)
#define MRC(expr)                                   \
    do {                                            \
        int _rc = (expr);                           \
        if (_rc) return _rc;                        \
    } while (0)

namespace {

// the index as it is now, and the handle brought up to it: a new epoch holds
// no times, a rollback keeps those below the flushed count it left.  `flush`:
// the caller will read the events' rows (lx_index_view), else lx_index_peek
int follow(lx_mt *m, IndexView *iv, bool flush) {
    const int rc = flush ? lx_index_view(m->ix, iv) : lx_index_peek(m->ix, iv);
    if (rc) {
        m->err = lx_last_error(m->ix);
        return rc;
    }
    if (iv->shard_count > 1) return m->fail(LX_ERR_STATE, "MedianTime needs an unsharded index");
    if (iv->epoch_gen != m->epoch_gen) {
        if (iv->V > kMtMaxV) return m->fail(LX_ERR_ARG, "MedianTime supports up to %u validators", kMtMaxV);
        m->V = iv->V;
        m->n_times = 0;
        m->epoch_gen = iv->epoch_gen;
    } else if (iv->roll_gen != m->roll_gen) {
        m->n_times = std::min(m->n_times, lx_index_kept_since(m->ix, m->roll_gen));
    }
    m->roll_gen = iv->roll_gen;
    int cur = -1;   // (hipSetDevice costs microseconds: only when the device is not current)
    if (hipGetDevice(&cur) != hipSuccess || cur != iv->device) MHIP(m, hipSetDevice(iv->device));
    return 0;
}

int query(lx_mt *m, uint32_t n, const uint32_t *ev, uint64_t default_time, uint64_t *median, uint64_t *merged) {
    if (!m) return LX_ERR_ARG;
    if (n && (!ev || (!median && !merged))) return m->fail(LX_ERR_ARG, "null argument");
    if (!n) return 0;
    IndexView iv;
    MRC(follow(m, &iv, true));
    if (iv.loading) return m->fail(LX_ERR_STATE, "index is loading (lx_load_finish first)");
    // (an index dropped by a rollback is both: it answers "time not set")
    for (uint32_t i = 0; i < n; i++) {
        if (ev[i] >= m->n_times) return m->fail(LX_ERR_STATE, "time not set for event %u", ev[i]);
        if (ev[i] >= iv.n_events) return m->fail(LX_ERR_ARG, "unknown event %u", ev[i]);
    }
    MtArgs a{};
    a.hb = iv.hb;
    a.stride = iv.stride;
    a.V = m->V;
    a.forks = iv.B > iv.V ? 1u : 0u;
    a.cheat_of = iv.cheat_of;
    a.cheat_off = iv.cheat_off;
    a.cheat_br = iv.cheat_br;
    a.weights = iv.wpad;
    a.brow = iv.brow;
    a.branch_first = iv.branch_first;
    a.s_cap = iv.s_cap;
    a.times = m->times;
    a.n_times = m->n_times;
    a.default_time = default_time;
    const uint32_t chunk =
        merged ? (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(kMtChunk, kMtRowBytes / (8ull * m->V))) : kMtChunk;
    for (uint32_t lo = 0; lo < n; lo += chunk) {
        const uint32_t c = std::min(chunk, n - lo);
        a.n = c;
        a.ev = nullptr;
        if (c <= kMtInline) {
            memcpy(a.iev, ev + lo, c * 4ull);
        } else {
            // (every launch that read the old buffer has been waited for below)
            MHIP(m, m->d_ev.grow(std::max<uint64_t>(c, 1024)));
            MHIP(m, hipMemcpyAsync(m->d_ev, ev + lo, c * 4ull, hipMemcpyHostToDevice, iv.stream));
            a.ev = m->d_ev;
        }
        if (median) {
            MHIP(m, m->med.grow(c, std::max<uint64_t>(c, 256), nullptr, false));
            a.median = m->med.dev();
        } else {
            MHIP(m, m->d_rows.grow((uint64_t)c * m->V));
            a.merged = m->d_rows;
        }
        MHIP(m, lx::launch_mt(a, iv.stream));
        if (merged)
            MHIP(m, hipMemcpyAsync(merged + (uint64_t)lo * m->V, m->d_rows, (uint64_t)c * m->V * 8, hipMemcpyDeviceToHost,
                                   iv.stream));
        MHIP(m, hipStreamSynchronize(iv.stream));
        if (median) memcpy(median + lo, m->med.host(), c * 8ull);
    }
    return 0;
}

}  // namespace

extern "C" {

int lx_mt_create(lx_index *index, lx_mt **out) {
    if (!index || !out) return LX_ERR_ARG;
    lx_mt *m = new lx_mt();
    m->ix = index;
    const int rc = lx_mt_reset(m);
    if (rc) {
        lx_mt_destroy(m);
        return rc;
    }
    *out = m;
    return 0;
}

void lx_mt_destroy(lx_mt *m) { delete m; }   // (every launch was waited for by the call that made it)

const char *lx_mt_last_error(const lx_mt *m) { return m ? m->err.c_str() : "null handle"; }

int lx_mt_reset(lx_mt *m) {
    if (!m) return LX_ERR_ARG;
    m->epoch_gen = ~0ull;   // no generation of the index: follow() takes the epoch over
    IndexView iv;
    return follow(m, &iv, false);
}

int lx_mt_set_times(lx_mt *m, uint64_t first_event, uint64_t n, const uint64_t *creation_time) {
    if (!m) return LX_ERR_ARG;
    if (n && !creation_time) return m->fail(LX_ERR_ARG, "null argument");
    IndexView iv;
    MRC(follow(m, &iv, false));
    if (first_event > m->n_times)
        return m->fail(LX_ERR_ARG, "times of events %llu.. would leave a hole (%llu held)", (unsigned long long)first_event,
                       (unsigned long long)m->n_times);
    if (first_event + n < first_event || first_event + n > 0xFFFFFFFFull)
        return m->fail(LX_ERR_ARG, "dense indices are 32-bit");
    if (!n) return 0;
    const uint64_t end = first_event + n;
    if (end > m->times.cap())
        MHIP(m, m->times.regrow(std::max<uint64_t>({end, 2 * m->times.cap(), 4096}), m->n_times, lxi::Fill::none, iv.stream));
    // queries run on the same stream; the caller's buffer is free on return
    MHIP(m, hipMemcpyAsync(m->times + first_event, creation_time, n * 8, hipMemcpyHostToDevice, iv.stream));
    MHIP(m, hipStreamSynchronize(iv.stream));
    m->n_times = std::max(m->n_times, end);
    return 0;
}

uint64_t lx_mt_num_times(lx_mt *m) {
    if (!m) return 0;
    IndexView iv;
    if (follow(m, &iv, false)) return 0;
    return m->n_times;
}

int lx_mt_median_time(lx_mt *m, uint32_t n, const uint32_t *ev, uint64_t default_time, uint64_t *out) {
    if (m && n && !out) return m->fail(LX_ERR_ARG, "null argument");
    return query(m, n, ev, default_time, out, nullptr);
}

int lx_mt_merged_times(lx_mt *m, uint32_t n, const uint32_t *ev, uint64_t *out) {
    if (m && n && !out) return m->fail(LX_ERR_ARG, "null argument");
    return query(m, n, ev, 0, nullptr, out);
}

}  // extern "C"
