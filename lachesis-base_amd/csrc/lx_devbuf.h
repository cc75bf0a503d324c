// lx_devbuf.h -- the one owner of device and pinned host memory of the host
// engine (lx_index.h and its neighbours).  A DevBuf frees what it holds when
// it is reset, moved over or destroyed, and grows in the two ways the engine
// needs: contents dropped, contents kept.  The memory backend M is a
// parameter so that pinned memory uses the same type and so that the type is
// tested on the CPU (tests/csrc/devbuf_harness.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
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

#ifdef __HIP__
template <typename T>
using PinBuf = DevBuf<T, PinnedMem<hipHostMallocDefault>>;   // pinned host memory
template <typename T>
using MapBuf = DevBuf<T, PinnedMem<hipHostMallocMapped>>;    // pinned and mapped into the device's address space
#endif

}  // namespace lxi
