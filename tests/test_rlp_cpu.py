"""The RLP writer and reader of BranchesInfo (lachesis-base_amd/csrc/lx_rlp.h)
on the CPU, through tests/csrc/rlp_harness.cpp: the encoding equals
oracle/rlp.py's at every header form (uint widths, short and long lists), it
decodes back to the same tables, and malformed input is refused.  The harness
hands the reader a copy of the input in a block of exactly its length; that the
reader stays inside it is what tests/csrc/rlp_selftest.cpp shows under the
address sanitizer (make rlp_selftest)."""

import ctypes
import os

import numpy as np
import pytest

from oracle import rlp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "lachesis-base_amd", "build")

U32P = ctypes.POINTER(ctypes.c_uint32)
U8P = ctypes.POINTER(ctypes.c_uint8)


@pytest.fixture(scope="module")
def lib():
    L = ctypes.CDLL(os.path.join(BUILD, "librlp_harness.so"))
    L.rlp_encode_bi.restype = ctypes.c_uint64
    L.rlp_encode_bi.argtypes = [ctypes.c_uint32, U32P, U32P, ctypes.c_uint32, U32P, U32P, U8P, ctypes.c_uint64]
    L.rlp_decode_bi.restype = ctypes.c_int
    L.rlp_decode_bi.argtypes = [U8P, ctypes.c_uint32, ctypes.c_uint32, U32P, U32P, ctypes.c_uint32, U32P,
                                ctypes.c_uint32, U32P, U32P]
    return L


def u32(x):
    return np.ascontiguousarray(x, dtype=np.uint32)


def ptr(a, t=U32P):
    return a.ctypes.data_as(t)


def encode(L, last, creator, by):
    off = u32(np.concatenate([[0], np.cumsum([len(x) for x in by])]))
    flat = u32([b for x in by for b in x] or [0])
    la, cr = u32(last or [0]), u32(creator or [0])
    n = L.rlp_encode_bi(len(last), ptr(la), ptr(cr), len(by), ptr(off), ptr(flat), None, 0)
    out = np.zeros(max(int(n), 1), dtype=np.uint8)
    assert L.rlp_encode_bi(len(last), ptr(la), ptr(cr), len(by), ptr(off), ptr(flat), ptr(out, U8P), n) == n
    return out[:n].tobytes()


def decode(L, data, cap=4096):
    buf = np.frombuffer(bytes(data) or b"\0", dtype=np.uint8).copy()
    last, cr, by = (np.zeros(cap, dtype=np.uint32) for _ in range(3))
    off = np.zeros(cap + 1, dtype=np.uint32)
    counts = np.zeros(4, dtype=np.uint32)
    r = L.rlp_decode_bi(ptr(buf, U8P), len(data), cap, ptr(last), ptr(cr), cap, ptr(off), cap, ptr(by), ptr(counts))
    assert r in (0, 1)
    if not r:
        return None
    nb, nc, nv, _ = (int(x) for x in counts)
    return (last[:nb].tolist(), cr[:nc].tolist(), [by[off[v]:off[v + 1]].tolist() for v in range(nv)])


UINTS = [0, 0x7F, 0x80, 0xFF, 0x100, 0xFFFFFF, 0x1000000, 0xFFFFFFFF]
TABLES = {
    "uint_widths": (UINTS, list(range(8)), [[i] for i in range(8)]),
    "uints_as_creators_and_branches": ([1] * 8, UINTS, [[u] for u in UINTS]),
    "payload_55": ([1] * 55, list(range(55)), [[i] for i in range(55)]),
    "payload_56": ([1] * 56, list(range(56)), [[i] for i in range(56)]),
    "sixty_branches": ([200] * 60, list(range(60)), [[i] for i in range(60)]),
    "three_branches_of_one_creator": ([3, 5, 2, 7, 9], [0, 1, 2, 1, 1], [[0], [1, 3, 4], [2]]),
    "example": ([3, 0, 2], [0, 1, 0], [[0, 2], [1]]),
    "empty": ([], [], []),
}
EXAMPLE = bytes.fromhex("ce" + "c3038002" + "c3800180" + "c5c28002c101")


@pytest.mark.parametrize("name", sorted(TABLES))
def test_encoding_equals_oracle_and_round_trips(lib, name):
    last, creator, by = TABLES[name]
    want = rlp.encode_branches_info(last, creator, by)
    got = encode(lib, last, creator, by)
    assert got == want
    assert decode(lib, got) == (last, creator, by)


def test_header_forms_are_the_ones_meant(lib):
    """the cases reach the headers they are named for"""
    assert encode(lib, *TABLES["example"]) == EXAMPLE
    assert rlp.encode([1] * 55)[0] == 0xC0 + 55 and rlp.encode([1] * 56)[:2] == bytes([0xF8, 56])
    assert encode(lib, *TABLES["sixty_branches"])[0] == 0xF9
    e = encode(lib, *TABLES["uint_widths"])
    for u in UINTS:
        assert rlp.enc_uint(u) in e


REFUSED = {
    "empty": b"",
    "trailing_byte": EXAMPLE + b"\x00",
    "string_for_outer_list": bytes([0x80 + len(EXAMPLE) - 1]) + EXAMPLE[1:],
    "string_for_inner_list": bytes.fromhex("ce" + "83038002" + "c3800180" + "c5c28002c101"),
    "string_for_creator_branches": bytes.fromhex("ce" + "c3038002" + "c3800180" + "c5828002c101"),
    "five_byte_uint": rlp.enc_list([rlp.enc_list([bytes.fromhex("850100000000")]), rlp.enc_list([b"\x80"]),
                                    rlp.enc_list([rlp.enc_list([b"\x80"])])]),
    "long_string_length_past_end": bytes.fromhex("ce" + "c3b9ffff" + "c3800180" + "c5c28002c101"),
    "long_list_length_past_end": bytes.fromhex("f9ffff") + EXAMPLE[1:],
    "long_list_length_bytes_past_end": bytes.fromhex("fb0000"),
    "list_length_ff_x8": bytes([0xFF]) + b"\xff" * 8 + EXAMPLE[1:],
    "inner_list_length_ff_x8": bytes([0xC0 + 9 + 14]) + bytes([0xFF]) + b"\xff" * 8 + EXAMPLE[1:],
    # two inner headers of eight 0xFF length bytes, the second starting on the last length byte of the
    # first (hl + len wraps to 8), then an empty long-form list: a reader that adds hl + len before it
    # compares takes this for three empty lists and accepts it
    "wrapped_lengths_read_as_empty_lists": bytes([0xC0 + 25]) + b"\xff" * 17 + b"\x00" * 8,
}
REFUSED.update({"prefix_%d" % k: EXAMPLE[:k] for k in range(1, len(EXAMPLE))})


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_malformed_input_is_refused(lib, name):
    assert decode(lib, REFUSED[name]) is None
