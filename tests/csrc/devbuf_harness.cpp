// devbuf_harness.cpp -- CPU test harness of the owning buffer type
// (lachesis-base_amd/csrc/lx_devbuf.h) over a host memory backend, for
// tests/test_devbuf_cpu.py.  Plain g++, no HIP.  Test infrastructure only.
//
// The backend counts live blocks and its own calls (allocations, fills, copies
// and waits, in the order they are made) and fails the k-th of them when told
// to.  The pooled buffer (BlockPool, PoolBuf) runs over the same backend, with
// byte elements so that the sizes of the test are the sizes of the blocks.
// -DDEVBUF_MAIN adds a main() that walks the same properties the Python
// test asserts: a stand-alone program for a run under the host sanitizers
// (g++ -fsanitize=address,undefined -DDEVBUF_MAIN).
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../lachesis-base_amd/csrc/lx_devbuf.h"

namespace {

struct HostMem {
    using err_t = int;
    using stream_t = int;
    static long live, ops, fail_at, syncs;
    static bool step() { return ++ops == fail_at; }
    static err_t alloc(void **p, size_t bytes) {
        if (step()) return 2;
        *p = malloc(bytes);
        memset(*p, 0xA5, bytes);   // a fresh block never reads as zeros by luck
        live++;
        return 0;
    }
    static void free(void *p) {
        ::free(p);
        live--;
    }
    static err_t copy(void *d, const void *s, size_t bytes, stream_t) {
        if (step()) return 3;
        memcpy(d, s, bytes);
        return 0;
    }
    static err_t zero(void *p, size_t bytes, stream_t) {
        if (step()) return 4;
        memset(p, 0, bytes);
        return 0;
    }
    static err_t sync(stream_t) {
        if (step()) return 5;
        syncs++;
        return 0;
    }
};
long HostMem::live = 0, HostMem::ops = 0, HostMem::fail_at = 0, HostMem::syncs = 0;

using Buf = lxi::DevBuf<uint32_t, HostMem>;
struct Several {
    Buf a, b, c;
    lxi::DevBuf<uint8_t, HostMem> bytes;
};

using Pool = lxi::BlockPool<HostMem>;
using PBuf = lxi::PoolBuf<uint8_t, HostMem>;
struct SeveralPooled {
    PBuf a, b;
    lxi::PoolBuf<uint32_t, HostMem> words;
};

}  // namespace

extern "C" {

long db_live() { return HostMem::live; }
long db_ops() { return HostMem::ops; }
long db_syncs() { return HostMem::syncs; }
// the k-th backend call from now on fails (0: none)
void db_fail_at(long k) {
    HostMem::ops = 0;
    HostMem::fail_at = k;
}
void *db_new() { return new Buf(); }
void db_delete(void *b) { delete static_cast<Buf *>(b); }
const void *db_ptr(void *b) { return static_cast<Buf *>(b)->get(); }
uint64_t db_cap(void *b) { return static_cast<Buf *>(b)->cap(); }
int db_grow(void *b, uint64_t need, int wait) { return static_cast<Buf *>(b)->grow(need, 0, wait != 0); }
int db_renew(void *b, uint64_t n, int wait) { return static_cast<Buf *>(b)->renew(n, 0, wait != 0); }
int db_regrow(void *b, uint64_t n, uint64_t keep, int fill) {
    return static_cast<Buf *>(b)->regrow(n, keep, static_cast<lxi::Fill>(fill), 0);
}
void db_reset(void *b) { static_cast<Buf *>(b)->reset(); }
void db_move(void *dst, void *src) { *static_cast<Buf *>(dst) = std::move(*static_cast<Buf *>(src)); }
void db_write(void *b, uint64_t i, uint32_t v) { static_cast<Buf *>(b)->get()[i] = v; }
uint32_t db_read(void *b, uint64_t i) { return (*static_cast<Buf *>(b))[i]; }
// a struct of several buffers, filled and destroyed at once: live blocks while it stands
long db_several(uint64_t n) {
    Several s;
    if (s.a.renew(n) || s.b.grow(2 * n) || s.c.regrow(n, 0, lxi::Fill::all, 0) || s.bytes.renew(3)) return -1;
    Several t = std::move(s);
    return HostMem::live;
}

// ---- the pooled buffer
void *pl_new() { return new Pool(); }
void pl_delete(void *p) { delete static_cast<Pool *>(p); }
void pl_drain(void *p) { static_cast<Pool *>(p)->drain(); }
long pl_idle(void *p) { return (long)static_cast<Pool *>(p)->idle(); }
void *pb_new() { return new PBuf(); }
void pb_delete(void *b) { delete static_cast<PBuf *>(b); }
const void *pb_ptr(void *b) { return static_cast<PBuf *>(b)->get(); }
uint64_t pb_cap(void *b) { return static_cast<PBuf *>(b)->cap(); }
int pb_regrow(void *b, void *pool, uint64_t n, uint64_t keep) {
    return static_cast<PBuf *>(b)->regrow(*static_cast<Pool *>(pool), n, keep, 0);
}
void pb_release(void *b) { static_cast<PBuf *>(b)->release(); }
void pb_move(void *dst, void *src) { *static_cast<PBuf *>(dst) = std::move(*static_cast<PBuf *>(src)); }
void pb_write(void *b, uint64_t i, uint8_t v) { static_cast<PBuf *>(b)->get()[i] = v; }
uint8_t pb_read(void *b, uint64_t i) { return (*static_cast<PBuf *>(b))[i]; }
// a struct of pooled buffers destroyed ahead of its pool, then the pool: live
// blocks while the struct stands, once it is gone, once the pool is gone
void pb_struct_then_pool(uint64_t n, long *standing, long *pooled, long *gone) {
    {
        Pool pool;
        {
            SeveralPooled s;
            if (s.a.regrow(pool, n, 0, 0) || s.b.regrow(pool, 2 * n, 0, 0) || s.words.regrow(pool, n, 0, 0)) return;
            SeveralPooled t = std::move(s);
            *standing = HostMem::live;
        }
        *pooled = HostMem::live;
    }
    *gone = HostMem::live;
}

}  // extern "C"

#ifdef DEVBUF_MAIN
#define CHECK(x)                                                      \
    do {                                                              \
        if (!(x)) {                                                   \
            printf("devbuf: line %d: %s\n", __LINE__, #x);            \
            return 1;                                                 \
        }                                                             \
    } while (0)

int main() {
    {
        Buf b;
        CHECK(b.grow(0) == 0 && b.get() && b.cap() == 0 && HostMem::live == 1);   // an empty request holds one element
        b.get()[0] = 7;
        CHECK(b.grow(0) == 0 && b.get()[0] == 7);                                 // large enough: untouched
        CHECK(b.grow(100, 0, true) == 0 && b.cap() == 100 && HostMem::syncs == 1 && HostMem::live == 1);
        for (uint32_t i = 0; i < 100; i++) b.get()[i] = i;
        const uint32_t *p = b;
        CHECK(b.grow(50) == 0 && b.get() == p && b.cap() == 100);
        CHECK(b.regrow(300, 100, lxi::Fill::tail, 0) == 0 && b.cap() == 300);
        for (uint32_t i = 0; i < 300; i++) CHECK(b[i] == (i < 100 ? i : 0u));
        CHECK(b.regrow(400, 10, lxi::Fill::none, 0) == 0 && b[9] == 9 && b[10] == 0xA5A5A5A5u);
        CHECK(b.regrow(500, 10, lxi::Fill::all, 0) == 0 && b[9] == 9 && b[10] == 0 && b[499] == 0);
        // every failure point of a regrow: the buffer is as it was
        for (long k = 1;; k++) {
            p = b;
            db_fail_at(k);
            const int rc = b.regrow(600, 10, lxi::Fill::tail, 0);
            db_fail_at(0);
            if (!rc) {
                CHECK(k == 5 && b.cap() == 600);   // alloc, fill, copy, wait
                break;
            }
            CHECK(b.get() == p && b.cap() == 500 && b[9] == 9 && b[10] == 0 && HostMem::live == 1);
        }
        Buf c = std::move(b);
        CHECK(!b.get() && b.cap() == 0 && c.cap() == 600 && HostMem::live == 1);
        b = std::move(c);
        CHECK(!c.get() && b.cap() == 600 && HostMem::live == 1);
        b.reset();
        CHECK(HostMem::live == 0 && !b.get() && b.cap() == 0);
    }
    CHECK(db_several(10) == 4 && HostMem::live == 0);
    {
        Pool pool;
        PBuf b, c;
        CHECK(b.regrow(pool, 1000, 0, 0) == 0 && b.cap() == 1000 && HostMem::live == 1);
        const uint8_t *p = b;
        // a released block comes back for the same size and for a smaller one, with no backend call
        b.release();
        CHECK(!b.get() && b.cap() == 0 && pool.idle() == 1 && HostMem::live == 1);
        db_fail_at(0);
        CHECK(b.regrow(pool, 1000, 0, 0) == 0 && b.get() == p && HostMem::ops == 0);
        b.release();
        CHECK(b.regrow(pool, 200, 0, 0) == 0 && b.get() == p && b.cap() == 1000 && HostMem::ops == 0);
        // 400,000 > 4 * 1,000 + 65,536: refused, a fresh block instead
        CHECK(c.regrow(pool, 400000, 0, 0) == 0);
        c.release();
        CHECK(c.regrow(pool, 1000, 0, 0) == 0 && c.cap() == 1000 && pool.idle() == 1 && HostMem::live == 3);
        pool.drain();
        CHECK(pool.idle() == 0 && HostMem::live == 2);
        // of two free blocks the smallest sufficient one
        b.release();
        c.release();
        CHECK(b.regrow(pool, 3000, 0, 0) == 0 && c.regrow(pool, 2000, 0, 0) == 0);
        const uint8_t *p3 = b, *p2 = c;
        b.release();
        c.release();
        CHECK(b.regrow(pool, 1500, 0, 0) == 0 && b.get() == p2 && b.cap() == 2000);
        CHECK(c.regrow(pool, 2500, 0, 0) == 0 && c.get() == p3 && c.cap() == 3000);
        // a grow that keeps a prefix: copied, the old block pooled, no wait
        for (uint32_t i = 0; i < 2000; i++) b.get()[i] = (uint8_t)(i * 7);
        const long syncs = HostMem::syncs, idle = (long)pool.idle();
        CHECK(b.regrow(pool, 100000, 2000, 0) == 0 && b.get() != p2 && b.cap() == 100000);
        CHECK(HostMem::syncs == syncs && (long)pool.idle() == idle + 1);
        for (uint32_t i = 0; i < 2000; i++) CHECK(b[i] == (uint8_t)(i * 7));
        // a failed allocation and a failed copy leave the buffer as it was; the
        // block of the failed copy is the pool's, not lost
        p = b;
        long live = HostMem::live;
        db_fail_at(1);
        CHECK(b.regrow(pool, 10000000, 2000, 0) != 0 && b.get() == p && b.cap() == 100000 && HostMem::live == live);
        db_fail_at(2);
        CHECK(b.regrow(pool, 10000000, 2000, 0) != 0 && b.get() == p && b.cap() == 100000);
        CHECK(HostMem::live == live + 1 && (long)pool.idle() == idle + 2);
        db_fail_at(1);   // the block now comes from the pool: the copy is the first call
        CHECK(b.regrow(pool, 10000000, 2000, 0) != 0 && b.get() == p && HostMem::live == live + 1);
        CHECK((long)pool.idle() == idle + 2);
        db_fail_at(0);
        PBuf d = std::move(b);   // moved over: c's block goes to the pool
        c = std::move(d);
        CHECK(!b.get() && !d.get() && c.get() == p && (long)pool.idle() == idle + 3);
        pool.drain();
        CHECK(HostMem::live == 1);
    }
    CHECK(HostMem::live == 0);
    long standing = -1, pooled = -1, gone = -1;
    pb_struct_then_pool(100, &standing, &pooled, &gone);
    CHECK(standing == 3 && pooled == 3 && gone == 0);
    printf("devbuf ok\n");
    return 0;
}
#endif
