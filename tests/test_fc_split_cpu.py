"""The column split of a k_root_fc launch (lachesis-base_amd/csrc/lx_fc_split.h)
on the CPU, against the formula restated here:

    s         = ceil(1024 / tiles), clamped to [1, max(ncols / 128, 1)]
    col_split = round_up(ceil(ncols / s), 32)
    n_split   = ceil(ncols / col_split)

tests/csrc/fc_split_harness.cpp exposes the header's functions."""

import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "lachesis-base_amd", "build")

NCOLS = [32, 128, 160, 384, 1024, 1056]
TILES = [1, 3, 512, 1024, 5000]


@pytest.fixture(scope="module")
def L():
    lib = ctypes.CDLL(os.path.join(BUILD, "libfc_split_harness.so"))
    lib.fs_col_split.restype = None
    lib.fs_col_split.argtypes = [ctypes.c_uint64, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32),
                                 ctypes.POINTER(ctypes.c_uint32)]
    lib.fs_tiles.restype = ctypes.c_uint64
    lib.fs_tiles.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
    return lib


def ceil_div(a, b):
    return -(-a // b)


def model(tiles, ncols):
    s = min(max(ceil_div(1024, tiles), 1), max(ncols // 128, 1))
    col_split = ceil_div(ceil_div(ncols, s), 32) * 32
    return col_split, ceil_div(ncols, col_split)


def split(L, tiles, ncols):
    cs, ns = ctypes.c_uint32(), ctypes.c_uint32()
    L.fs_col_split(tiles, ncols, ctypes.byref(cs), ctypes.byref(ns))
    return cs.value, ns.value


@pytest.mark.parametrize("ncols", NCOLS)
@pytest.mark.parametrize("tiles", TILES)
def test_split_is_the_formula(L, tiles, ncols):
    col_split, n_split = split(L, tiles, ncols)
    assert (col_split, n_split) == model(tiles, ncols)
    assert col_split % 32 == 0 and col_split > 0
    assert n_split * col_split >= ncols            # every column is in a split
    assert (n_split - 1) * col_split < ncols       # and every split holds one


def test_edges(L):
    for tiles in TILES:
        assert split(L, tiles, 32) == (32, 1)      # fewer than 128 columns: one split
    # 8 splits asked of 1056 columns: 132 columns each, rounded up to 160, leave 7
    assert split(L, 1, 1056) == (160, 7)
    assert split(L, 1, 1024) == (128, 8)
    assert split(L, 5000, 1056) == (1056, 1)       # the tiles fill the chip: no split


def test_tiles_of_a_step(L):
    for n_cand, n_roots, want in [(1, 1, 1), (64, 64, 1), (65, 64, 2), (65, 129, 6), (1000, 1, 16)]:
        assert L.fs_tiles(n_cand, n_roots) == want
