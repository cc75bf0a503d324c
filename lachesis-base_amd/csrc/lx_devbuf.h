// lx_devbuf.h -- the one owner of device and pinned host memory of the host
// engine (lx_index.h and its neighbours).  A DevBuf frees what it holds when
// it is reset, moved over or destroyed, and grows in the two ways the engine
// needs: contents dropped, contents kept.  The memory backend M is a
// parameter so that pinned memory uses the same type and so that the type is
// tested on the CPU (tests/csrc/devbuf_harness.cpp).  BlockPool and PoolBuf are
// the same for buffers that come and go too often to be allocated each time
// (the abft engine's), MappedBuf for pinned memory a kernel writes into.
#pragma once
#include <cstddef>
#include <cstdint>
#include <map>
#include <utility>

#ifdef __HIP__
#include <hip/hip_runtime.h>
#endif

namespace lxi {

#ifdef __HIP__
// device memory; copies, fills and waits on a HIP stream
struct DeviceMem {
    using err_t = hipError_t;
    using stream_t = hipStream_t;
    static err_t alloc(void **p, size_t bytes) { return hipMalloc(p, bytes); }
    static void free(void *p) { (void)hipFree(p); }
    static err_t copy(void *d, const void *s, size_t bytes, stream_t st) {
        return hipMemcpyAsync(d, s, bytes, hipMemcpyDeviceToDevice, st);
    }
    static err_t zero(void *p, size_t bytes, stream_t st) { return hipMemsetAsync(p, 0, bytes, st); }
    static err_t sync(stream_t st) { return hipStreamSynchronize(st); }
};
// pinned host memory (Flags: hipHostMallocDefault, hipHostMallocMapped)
template <unsigned Flags>
struct PinnedMem : DeviceMem {
    static err_t alloc(void **p, size_t bytes) { return hipHostMalloc(p, bytes, Flags); }
    static void free(void *p) { (void)hipHostFree(p); }
};
#define LX_DEVBUF_DEFAULT_MEM = DeviceMem
#else
#define LX_DEVBUF_DEFAULT_MEM
#endif

enum class Fill { none, tail, all };   // regrow: zero nothing, the elements past `keep`, or the whole new block

template <typename T, typename M LX_DEVBUF_DEFAULT_MEM>
class DevBuf {
    T *p_ = nullptr;
    uint64_t cap_ = 0;   // elements asked for (an empty request still holds one element)

public:
    using err_t = typename M::err_t;
    using stream_t = typename M::stream_t;

    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr, o.cap_ = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) {
            reset();
            std::swap(p_, o.p_);
            std::swap(cap_, o.cap_);
        }
        return *this;
    }
    ~DevBuf() { reset(); }

    // implicit, so that kernel-argument code reads `t.la = h->la` and `brow + x`
    // as with a raw pointer; the price is that `delete buf` would compile too:
    // a DevBuf is never deleted or freed by hand
    operator T *() const { return p_; }
    T *get() const { return p_; }
    uint64_t cap() const { return cap_; }
    uint64_t bytes() const { return cap_ * sizeof(T); }

    void reset() {
        if (p_) M::free(p_);
        p_ = nullptr;
        cap_ = 0;
    }

    // A fresh block of n elements, contents undefined: the old block is freed
    // first (after a wait for the stream when `wait`).  A failed wait leaves
    // the buffer as it was, a failed allocation leaves it empty.
    err_t renew(uint64_t n, stream_t st = {}, bool wait = false) {
        if (p_ && wait)
            if (err_t e = M::sync(st)) return e;
        reset();
        void *q = nullptr;
        if (err_t e = M::alloc(&q, (n ? n : 1) * sizeof(T))) return e;
        p_ = static_cast<T *>(q);
        cap_ = n;
        return err_t{};
    }

    // Contents dropped: nothing to do when the block holds `need` elements
    // already, else renew.
    err_t grow(uint64_t need, stream_t st = {}, bool wait = false) {
        if (cap_ >= need && p_) return err_t{};
        return renew(need, st, wait);
    }

    // Contents kept: a new block of n elements, zero-filled as `fill` says,
    // takes the first `keep` elements on the stream; the old block, if there
    // is one, is freed after a wait for the stream.  If any step fails the new
    // block is freed and the buffer is as it was.
    err_t regrow(uint64_t n, uint64_t keep, Fill fill, stream_t st) {
        DevBuf nb;
        if (err_t e = nb.renew(n)) return e;
        if (!p_) keep = 0;
        const uint64_t z0 = fill == Fill::all ? 0 : keep;
        if (fill != Fill::none && n > z0)
            if (err_t e = M::zero(nb.p_ + z0, (n - z0) * sizeof(T), st)) return e;
        if (keep)
            if (err_t e = M::copy(nb.p_, p_, keep * sizeof(T), st)) return e;
        if (p_)
            if (err_t e = M::sync(st)) return e;
        *this = std::move(nb);
        return err_t{};
    }
};

// Blocks recycled among the PoolBufs of one owner whose device work all runs
// on one stream: a block handed back can be taken again by later work on that
// stream without a wait (stream-ordered reuse).  The pool frees what it holds
// when it is drained or destroyed; declare it ahead of its buffers, so that it
// goes last.
template <typename M LX_DEVBUF_DEFAULT_MEM>
class BlockPool {
    std::multimap<uint64_t, void *> free_;   // bytes -> block

public:
    BlockPool() = default;
    BlockPool(const BlockPool &) = delete;
    BlockPool &operator=(const BlockPool &) = delete;
    ~BlockPool() { drain(); }

    void put(void *p, uint64_t bytes) {
        if (p) free_.emplace(bytes, p);
    }
    // the smallest free block of [bytes, 4 * bytes + 65536] bytes, or nullptr
    void *take(uint64_t bytes, uint64_t *got) {
        auto it = free_.lower_bound(bytes);
        if (it == free_.end() || it->first > 4 * bytes + 65536) return nullptr;
        void *p = it->second;
        *got = it->first;
        free_.erase(it);
        return p;
    }
    void drain() {
        for (auto &kv : free_) M::free(kv.second);
        free_.clear();
    }
    size_t idle() const { return free_.size(); }
};

// A DevBuf whose blocks come from and go back to a BlockPool: released, moved
// over or destroyed, it returns its block to the pool it was last grown from,
// without a wait (freed directly when it has none).
template <typename T, typename M LX_DEVBUF_DEFAULT_MEM>
class PoolBuf {
    T *p_ = nullptr;
    uint64_t cap_ = 0;
    BlockPool<M> *pool_ = nullptr;

public:
    using err_t = typename M::err_t;
    using stream_t = typename M::stream_t;

    PoolBuf() = default;
    PoolBuf(const PoolBuf &) = delete;
    PoolBuf &operator=(const PoolBuf &) = delete;
    PoolBuf(PoolBuf &&o) noexcept : p_(o.p_), cap_(o.cap_), pool_(o.pool_) { o.p_ = nullptr, o.cap_ = 0; }
    PoolBuf &operator=(PoolBuf &&o) noexcept {
        if (this != &o) {
            release();
            std::swap(p_, o.p_);
            std::swap(cap_, o.cap_);
            pool_ = o.pool_;
        }
        return *this;
    }
    ~PoolBuf() { release(); }

    operator T *() const { return p_; }   // as DevBuf: never deleted or freed by hand
    T *get() const { return p_; }
    uint64_t cap() const { return cap_; }
    uint64_t bytes() const { return cap_ * sizeof(T); }

    void release() {
        if (p_) {
            if (pool_) pool_->put(p_, cap_ * sizeof(T));
            else M::free(p_);
        }
        p_ = nullptr;
        cap_ = 0;
    }

    // A block of at least n elements (n > 0) from `pool`, or a fresh one when
    // the pool has none that fits; it takes the first `keep` elements on the
    // stream, and the old block goes back to its pool.  A failed allocation
    // leaves the buffer as it was; so does a failed copy, after which the new
    // block is the pool's.
    err_t regrow(BlockPool<M> &pool, uint64_t n, uint64_t keep, stream_t st) {
        uint64_t got = n * sizeof(T);
        void *q = pool.take(got, &got);
        if (!q)
            if (err_t e = M::alloc(&q, got)) return e;
        if (p_ && keep)
            if (err_t e = M::copy(q, p_, keep * sizeof(T), st)) {
                pool.put(q, got);
                return e;
            }
        release();
        p_ = static_cast<T *>(q);
        cap_ = got / sizeof(T);
        pool_ = &pool;
        return err_t{};
    }
};

#ifdef __HIP__
template <typename T>
using PinBuf = DevBuf<T, PinnedMem<hipHostMallocDefault>>;   // pinned host memory
template <typename T>
using MapBuf = DevBuf<T, PinnedMem<hipHostMallocMapped>>;    // pinned and mapped into the device's address space

// A MapBuf with the device's address of its block, asked once per allocation.
template <typename T>
class MappedBuf {
    MapBuf<T> h_;
    T *dev_ = nullptr;

public:
    T *host() const { return h_.get(); }
    T *dev() const { return dev_; }
    uint64_t cap() const { return h_.cap(); }
    // Contents dropped: nothing to do when the block holds `need` elements,
    // else a fresh block of `want` (the old one is freed first, after a wait
    // for the stream when `wait`).
    hipError_t grow(uint64_t need, uint64_t want, hipStream_t st, bool wait) {
        if (need <= h_.cap() && h_) return hipSuccess;
        if (hipError_t e = h_.renew(want, st, wait)) {
            if (!h_) dev_ = nullptr;
            return e;
        }
        void *d = nullptr;
        if (hipError_t e = hipHostGetDevicePointer(&d, h_.get(), 0)) {
            h_.reset();
            return e;
        }
        dev_ = static_cast<T *>(d);
        return hipSuccess;
    }
};

struct Event {   // a HIP event, destroyed with its owner
    hipEvent_t e = nullptr;
    Event() = default;
    Event(Event &&o) noexcept : e(o.e) { o.e = nullptr; }
    Event &operator=(Event &&) = delete;
    ~Event() {
        if (e) (void)hipEventDestroy(e);
    }
    operator hipEvent_t() const { return e; }
};

struct Stream {   // a HIP stream, destroyed with its owner (who waits for its work first)
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(Stream &&o) noexcept : s(o.s) { o.s = nullptr; }
    Stream &operator=(Stream &&) = delete;
    ~Stream() {
        if (s) (void)hipStreamDestroy(s);
    }
    operator hipStream_t() const { return s; }
};
#endif

}  // namespace lxi
