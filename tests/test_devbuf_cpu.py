"""The owning buffer type (lachesis-base_amd/csrc/lx_devbuf.h) on the CPU.

tests/csrc/devbuf_harness.cpp instantiates it over a host backend (malloc /
free / memcpy) that counts live blocks and fails the k-th of its calls
(allocation, fill, copy, wait) when told to.  The pooled buffer (BlockPool,
PoolBuf) runs over the same backend with byte elements."""

import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "lachesis-base_amd", "build")

FILL_NONE, FILL_TAIL, FILL_ALL = 0, 1, 2
FRESH = 0xA5A5A5A5          # what the backend writes into a new block


@pytest.fixture(scope="module")
def L():
    lib = ctypes.CDLL(os.path.join(BUILD, "libdevbuf_harness.so"))
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    for name, res, args in [
            ("db_live", ctypes.c_long, []), ("db_ops", ctypes.c_long, []), ("db_syncs", ctypes.c_long, []),
            ("db_fail_at", None, [ctypes.c_long]), ("db_new", vp, []), ("db_delete", None, [vp]),
            ("db_ptr", vp, [vp]), ("db_cap", u64, [vp]), ("db_grow", ctypes.c_int, [vp, u64, ctypes.c_int]),
            ("db_renew", ctypes.c_int, [vp, u64, ctypes.c_int]),
            ("db_regrow", ctypes.c_int, [vp, u64, u64, ctypes.c_int]), ("db_reset", None, [vp]),
            ("db_move", None, [vp, vp]), ("db_write", None, [vp, u64, ctypes.c_uint32]),
            ("db_read", ctypes.c_uint32, [vp, u64]), ("db_several", ctypes.c_long, [u64]),
            ("pl_new", vp, []), ("pl_delete", None, [vp]), ("pl_drain", None, [vp]), ("pl_idle", ctypes.c_long, [vp]),
            ("pb_new", vp, []), ("pb_delete", None, [vp]), ("pb_ptr", vp, [vp]), ("pb_cap", u64, [vp]),
            ("pb_regrow", ctypes.c_int, [vp, vp, u64, u64]), ("pb_release", None, [vp]), ("pb_move", None, [vp, vp]),
            ("pb_write", None, [vp, u64, ctypes.c_uint8]), ("pb_read", ctypes.c_uint8, [vp, u64]),
            ("pb_struct_then_pool", None, [u64] + [ctypes.POINTER(ctypes.c_long)] * 3)]:
        f = getattr(lib, name)
        f.restype, f.argtypes = res, args
    return lib


@pytest.fixture
def buf(L):
    assert L.db_live() == 0
    L.db_fail_at(0)
    b = L.db_new()
    yield b
    L.db_fail_at(0)
    L.db_delete(b)
    assert L.db_live() == 0


def fill(L, b, n):
    for i in range(n):
        L.db_write(b, i, 1000 + i)


def test_grow_drops_contents(L, buf):
    # an empty request still holds one element; its capacity is what was asked
    assert L.db_grow(buf, 0, 0) == 0
    assert L.db_ptr(buf) and L.db_cap(buf) == 0 and L.db_live() == 1
    p = L.db_ptr(buf)
    assert L.db_grow(buf, 0, 0) == 0 and L.db_ptr(buf) == p         # large enough: nothing happens
    assert L.db_grow(buf, 100, 0) == 0
    assert L.db_cap(buf) == 100 and L.db_live() == 1
    assert L.db_read(buf, 0) == FRESH and L.db_read(buf, 99) == FRESH
    fill(L, buf, 100)
    p, ops = L.db_ptr(buf), L.db_ops()
    for need in (1, 50, 100):
        assert L.db_grow(buf, need, 1) == 0
    assert (L.db_ptr(buf), L.db_cap(buf), L.db_ops()) == (p, 100, ops)   # no call into the backend at all
    assert L.db_read(buf, 99) == 1099
    # the wait comes before the old block is freed, only when asked and only when there is one
    s = L.db_syncs()
    assert L.db_grow(buf, 101, 0) == 0 and L.db_syncs() == s
    assert L.db_grow(buf, 102, 1) == 0 and L.db_syncs() == s + 1
    assert L.db_cap(buf) == 102 and L.db_live() == 1
    L.db_reset(buf)
    assert L.db_grow(buf, 5, 1) == 0 and L.db_syncs() == s + 1
    # a failed allocation leaves the buffer empty, a failed wait leaves it as it was
    L.db_fail_at(2)
    assert L.db_renew(buf, 7, 1) != 0
    assert not L.db_ptr(buf) and L.db_cap(buf) == 0 and L.db_live() == 0
    L.db_fail_at(0)
    assert L.db_renew(buf, 7, 1) == 0
    L.db_fail_at(1)
    assert L.db_renew(buf, 9, 1) != 0 and L.db_cap(buf) == 7 and L.db_live() == 1


@pytest.mark.parametrize("mode", [FILL_NONE, FILL_TAIL, FILL_ALL])
def test_regrow_keeps_prefix(L, buf, mode):
    assert L.db_regrow(buf, 64, 10, mode) == 0           # nothing to keep yet
    assert L.db_cap(buf) == 64 and L.db_live() == 1
    assert [L.db_read(buf, i) for i in (0, 9, 10, 63)] == [FRESH if mode == FILL_NONE else 0] * 4
    fill(L, buf, 64)
    s = L.db_syncs()
    assert L.db_regrow(buf, 200, 40, mode) == 0
    assert L.db_cap(buf) == 200 and L.db_live() == 1 and L.db_syncs() == s + 1
    assert [L.db_read(buf, i) for i in range(40)] == [1000 + i for i in range(40)]
    rest = {L.db_read(buf, i) for i in range(40, 200)}
    assert rest == ({FRESH} if mode == FILL_NONE else {0})          # (the old elements 40..63 are not kept)
    assert L.db_regrow(buf, 20, 20, mode) == 0                      # a smaller block keeps what fits
    assert [L.db_read(buf, i) for i in range(20)] == [1000 + i for i in range(20)]


@pytest.mark.parametrize("mode", [FILL_NONE, FILL_TAIL, FILL_ALL])
def test_regrow_failure_leaves_the_buffer(L, buf, mode):
    assert L.db_renew(buf, 32, 0) == 0
    fill(L, buf, 32)
    p = L.db_ptr(buf)
    steps = 3 if mode == FILL_NONE else 4                # allocation, (fill,) copy, wait
    for k in range(1, steps + 1):
        L.db_fail_at(k)
        assert L.db_regrow(buf, 100, 32, mode) != 0, k
        assert L.db_ptr(buf) == p and L.db_cap(buf) == 32 and L.db_live() == 1, k
        assert [L.db_read(buf, i) for i in range(32)] == [1000 + i for i in range(32)], k
    L.db_fail_at(steps + 1)                              # no further call to fail: it succeeds
    assert L.db_regrow(buf, 100, 32, mode) == 0 and L.db_ops() == steps
    assert L.db_cap(buf) == 100 and L.db_live() == 1
    assert [L.db_read(buf, i) for i in range(32)] == [1000 + i for i in range(32)]


def test_move_and_reset(L, buf):
    other = L.db_new()
    assert L.db_renew(buf, 8, 0) == 0 and L.db_renew(other, 16, 0) == 0
    L.db_write(other, 15, 77)
    p = L.db_ptr(other)
    assert L.db_live() == 2
    L.db_move(buf, other)                                # frees what buf held, empties other
    assert L.db_live() == 1
    assert L.db_ptr(buf) == p and L.db_cap(buf) == 16 and L.db_read(buf, 15) == 77
    assert not L.db_ptr(other) and L.db_cap(other) == 0
    L.db_move(buf, buf)
    assert L.db_ptr(buf) == p and L.db_live() == 1
    L.db_reset(buf)
    assert L.db_live() == 0 and not L.db_ptr(buf) and L.db_cap(buf) == 0
    L.db_reset(buf)
    L.db_delete(other)
    assert L.db_live() == 0


def test_struct_of_buffers_goes_at_once(L):
    assert L.db_live() == 0
    L.db_fail_at(0)
    assert L.db_several(10) == 4                         # four blocks while the struct stands
    assert L.db_live() == 0


# ---- the pooled buffer


@pytest.fixture
def pool(L):
    """A pool and two buffers; everything is gone afterwards, the pool last."""
    assert L.db_live() == 0
    L.db_fail_at(0)
    p, b, c = L.pl_new(), L.pb_new(), L.pb_new()
    yield p, b, c
    L.db_fail_at(0)
    L.pb_delete(b)
    L.pb_delete(c)
    L.pl_delete(p)
    assert L.db_live() == 0


def test_pool_hands_a_released_block_back(L, pool):
    p, b, _ = pool
    assert L.pb_regrow(b, p, 1000, 0) == 0
    assert L.pb_cap(b) == 1000 and L.db_live() == 1 and L.pl_idle(p) == 0
    ptr = L.pb_ptr(b)
    for want in (1000, 200):                       # the same size, a smaller one
        L.pb_release(b)
        assert not L.pb_ptr(b) and L.pb_cap(b) == 0
        assert L.pl_idle(p) == 1 and L.db_live() == 1          # pooled, not freed
        L.db_fail_at(0)
        assert L.pb_regrow(b, p, want, 0) == 0
        assert L.db_ops() == 0                                 # no call into the backend at all
        assert L.pb_ptr(b) == ptr and L.pb_cap(b) == 1000 and L.pl_idle(p) == 0


def test_pool_refuses_a_block_far_too_large(L, pool):
    p, b, c = pool
    assert L.pb_regrow(b, p, 400000, 0) == 0
    big = L.pb_ptr(b)
    L.pb_release(b)
    L.db_fail_at(0)
    assert L.pb_regrow(c, p, 1000, 0) == 0         # 400,000 > 4 * 1,000 + 65,536
    assert L.pb_ptr(c) != big and L.pb_cap(c) == 1000
    assert L.db_ops() == 1 and L.db_live() == 2 and L.pl_idle(p) == 1      # a fresh block; the large one stays
    # the bound itself: 4 * n + 65,536 = 400,000 at n = 83,616
    assert L.pb_regrow(b, p, 83615, 0) == 0 and L.pb_ptr(b) != big
    L.pb_release(c)
    assert L.pb_regrow(c, p, 83616, 0) == 0 and L.pb_ptr(c) == big and L.pb_cap(c) == 400000


def test_pool_takes_the_smallest_sufficient_block(L, pool):
    p, b, c = pool
    assert L.pb_regrow(b, p, 3000, 0) == 0 and L.pb_regrow(c, p, 2000, 0) == 0
    p3, p2 = L.pb_ptr(b), L.pb_ptr(c)
    L.pb_release(b)
    L.pb_release(c)
    assert L.pl_idle(p) == 2
    assert L.pb_regrow(b, p, 1500, 0) == 0
    assert L.pb_ptr(b) == p2 and L.pb_cap(b) == 2000
    L.pb_release(b)
    assert L.pb_regrow(b, p, 2001, 0) == 0         # the smaller one no longer suffices
    assert L.pb_ptr(b) == p3 and L.pb_cap(b) == 3000 and L.pl_idle(p) == 1


def test_pooled_grow_keeps_the_prefix_without_a_wait(L, pool):
    p, b, c = pool
    assert L.pb_regrow(b, p, 1000, 0) == 0
    for i in range(1000):
        L.pb_write(b, i, i * 7 % 251)
    old, s = L.pb_ptr(b), L.db_syncs()
    L.db_fail_at(0)
    assert L.pb_regrow(b, p, 5000, 600) == 0
    assert L.db_ops() == 2 and L.db_syncs() == s                # allocation and copy: nothing waits
    assert L.pb_ptr(b) != old and L.pb_cap(b) == 5000
    assert [L.pb_read(b, i) for i in range(600)] == [i * 7 % 251 for i in range(600)]
    assert L.pb_read(b, 600) == 0xA5                            # past the prefix: the fresh block
    assert L.pl_idle(p) == 1 and L.db_live() == 2               # the old block is the pool's
    assert L.pb_regrow(c, p, 1000, 0) == 0 and L.pb_ptr(c) == old


def test_pooled_grow_failure_leaves_the_buffer(L, pool):
    p, b, c = pool
    assert L.pb_regrow(b, p, 1000, 0) == 0
    for i in range(1000):
        L.pb_write(b, i, i % 200)
    ptr = L.pb_ptr(b)

    def unchanged():
        return (L.pb_ptr(b) == ptr and L.pb_cap(b) == 1000
                and [L.pb_read(b, i) for i in range(1000)] == [i % 200 for i in range(1000)])

    L.db_fail_at(1)                                # the allocation
    assert L.pb_regrow(b, p, 5000, 1000) != 0
    assert unchanged() and L.db_live() == 1 and L.pl_idle(p) == 0
    # the copy into a block taken from the pool: the block goes back, the counts are as they were
    assert L.pb_regrow(c, p, 5000, 0) == 0
    L.pb_release(c)
    assert L.db_live() == 2 and L.pl_idle(p) == 1
    L.db_fail_at(1)                                # no allocation now: the copy is the first call
    assert L.pb_regrow(b, p, 5000, 1000) != 0
    assert unchanged() and L.db_live() == 2 and L.pl_idle(p) == 1
    # the copy into a fresh block: that block is the pool's now, not lost (no block outside buffer and pool)
    L.db_fail_at(2)
    assert L.pb_regrow(b, p, 1000000, 1000) != 0
    assert unchanged() and L.pl_idle(p) == 2 and L.db_live() == 1 + L.pl_idle(p)
    L.db_fail_at(0)
    assert L.pb_regrow(b, p, 1000000, 1000) == 0 and L.db_ops() == 1       # that block, and the copy
    assert [L.pb_read(b, i) for i in range(1000)] == [i % 200 for i in range(1000)]
    L.pl_drain(p)
    assert L.pl_idle(p) == 0 and L.db_live() == 1


def test_drain_and_moves(L, pool):
    p, b, c = pool
    assert L.pb_regrow(b, p, 100, 0) == 0 and L.pb_regrow(c, p, 70000, 0) == 0
    ptr = L.pb_ptr(c)
    L.pb_move(b, c)                                # what b held goes to the pool, c is empty
    assert L.pb_ptr(b) == ptr and L.pb_cap(b) == 70000 and not L.pb_ptr(c) and L.pb_cap(c) == 0
    assert L.pl_idle(p) == 1 and L.db_live() == 2
    L.pb_move(b, b)
    assert L.pb_ptr(b) == ptr and L.db_live() == 2
    L.pb_release(b)
    L.pb_release(b)
    assert L.pl_idle(p) == 2
    L.pl_drain(p)
    assert L.pl_idle(p) == 0 and L.db_live() == 0
    # a buffer that never saw a pool frees directly
    fresh = L.pb_new()
    L.pb_release(fresh)
    L.pb_delete(fresh)
    assert L.db_live() == 0


def test_struct_of_pooled_buffers_then_the_pool(L):
    assert L.db_live() == 0
    L.db_fail_at(0)
    n = [ctypes.c_long(-1) for _ in range(3)]
    L.pb_struct_then_pool(100, *[ctypes.byref(x) for x in n])
    # three blocks while the struct stands; pooled when it is gone; freed with the pool
    assert [x.value for x in n] == [3, 3, 0]
    assert L.db_live() == 0
