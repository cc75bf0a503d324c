"""The owning buffer type (lachesis-base_amd/csrc/lx_devbuf.h) on the CPU.

tests/csrc/devbuf_harness.cpp instantiates it over a host backend (malloc /
free / memcpy) that counts live blocks and fails the k-th of its calls
(allocation, fill, copy, wait) when told to."""

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
            ("db_read", ctypes.c_uint32, [vp, u64]), ("db_several", ctypes.c_long, [u64])]:
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
