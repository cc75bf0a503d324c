"""The walker's three-input packed maximum (pk_max3_f16 of lx_internal.h:
v_pk_maximum3_f16 on raw seq words) against the integer maximum of both
16-bit halves, on the range the F3 fold is gated to, 0x0000..0x7BFF
(kFold3MaxSeq): the non-negative finite f16 bit patterns, denormals
(0x0001..0x03FF) included.  The kernels of tests/csrc/fold3_harness.cpp call
the same __forceinline__ helper as index_body.

* every pair (x, y) of the range in both halves of a word, the third operand
  zero, the zero in each of the three operand positions (3 x 31744^2 results,
  checked on the device, one launch);
* 2^24 seeded random triples of words (one launch, compared in numpy);
* every triple of the corners 0, 1, 0x03FF, 0x0400, 0x7BFF in the low half
  against every such triple in the high half (one launch, compared in numpy).

This test decides whether the F3 fold may ship: a single differing result
means a walk on such seqs could publish a wrong HighestBefore entry.

Measured on an MI355X: every pair 0.23 s, random triples 0.30-0.39 s, corners
under 0.01 s; all results equal.
"""

import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
u32p = ctypes.POINTER(ctypes.c_uint32)
u64p = ctypes.POINTER(ctypes.c_uint64)
LIM = 0x7C00            # seqs 0 .. kFold3MaxSeq
CORNERS = [0, 1, 0x03FF, 0x0400, 0x7BFF]
_lib = None


def lib():
    global _lib
    if _lib is None:
        L = ctypes.CDLL(os.path.join(os.path.dirname(HERE), "lachesis-base_amd", "build", "libfold3_harness.so"))
        L.f3h_last_error.restype = ctypes.c_char_p
        L.f3h_apply.argtypes = [u32p, u32p, u32p, ctypes.c_uint64, u32p]
        L.f3h_pairs.argtypes = [ctypes.c_uint32, u64p]
        _lib = L
    return _lib


def apply(a, b, c):
    a, b, c = (np.ascontiguousarray(x, dtype=np.uint32) for x in (a, b, c))
    out = np.zeros(len(a), dtype=np.uint32)
    rc = lib().f3h_apply(a.ctypes.data_as(u32p), b.ctypes.data_as(u32p), c.ctypes.data_as(u32p), len(a),
                         out.ctypes.data_as(u32p))
    assert rc == 0, lib().f3h_last_error()
    return out


def int_max3(a, b, c):
    """Integer maximum of the low and of the high halves."""
    lo = np.maximum(np.maximum(a & 0xFFFF, b & 0xFFFF), c & 0xFFFF)
    hi = np.maximum(np.maximum(a >> 16, b >> 16), c >> 16)
    return (lo | hi << 16).astype(np.uint32)


def check(a, b, c):
    got, want = apply(a, b, c), int_max3(a, b, c)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, "%d of %d differ, first: max3(%#x, %#x, %#x) = %#x, integer %#x" % (
        len(bad), len(a), a[bad[0]], b[bad[0]], c[bad[0]], got[bad[0]], want[bad[0]])


def test_every_pair_each_position():
    res = np.zeros(6, dtype=np.uint64)
    rc = lib().f3h_pairs(LIM, res.ctypes.data_as(u64p))
    assert rc == 0, lib().f3h_last_error()
    checked, bad, pos, x, y, got = (int(v) for v in res)
    assert checked == 3 * LIM * LIM
    assert bad == 0, "%d results differ, first: zero in position %d, halves (%#x, %#x) and (%#x, %#x): got %#x" % (
        bad, pos, x, y, y, x, got)


def test_random_triples():
    rng = np.random.default_rng(7)
    a, b, c = (rng.integers(0, LIM, 1 << 24, dtype=np.uint32) | rng.integers(0, LIM, 1 << 24, dtype=np.uint32) << 16
               for _ in range(3))
    check(a, b, c)


def test_corners():
    k = np.array(CORNERS, dtype=np.uint32)
    t = np.stack(np.meshgrid(k, k, k, indexing="ij"), -1).reshape(-1, 3)      # 125 triples of one half
    lo, hi = np.repeat(t, len(t), axis=0), np.tile(t, (len(t), 1))
    w = lo | hi << 16
    assert len(w) == 125 * 125
    check(w[:, 0], w[:, 1], w[:, 2])
