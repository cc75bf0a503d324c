"""The walk plan (lachesis-base_amd/csrc/lx_walk_plan.h) on the CPU: which
walker instance a batch takes, on what grid, as how many segments.

tests/csrc/walk_plan_harness.cpp exposes the header's functions over flat C
structs.  The model below is independent of the header: it is the rule set as
the host engine spelled it before the header existed, function by function
(walk_grid, seg_pick and auto_segments, the slice-width clamps of
add_batch_dev and seg_walk, launch_index and launch_index_t with its
8- / 12-column ladder and seg_xmap table).  Every field of the plan is compared
with it over a seeded sample of the cross product of the axes below; the
sample is asserted to reach every walker instance (the fourteen variants, each
as k_index and as k_index_segs), both outcomes of the one-launch test and a
non-empty seg_map."""

import ctypes
import itertools
import os
import random

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "lachesis-base_amd", "build")

IN_FIELDS = ["ncols", "V", "B", "max_seq", "n_cus", "sharded", "rowseg", "crec", "cpw", "pack16", "fold3", "seg_xmap",
             "seg_auto", "segments"]
OUT_FIELDS = ["cpw", "ncw", "nd", "masked", "packed", "crec", "fold3", "n_slices", "slices_per_xcd", "grid",
              "walk_cus", "G", "one_launch", "seg_grid", "seg_map_n"]


class WpIn(ctypes.Structure):
    _fields_ = [(f, ctypes.c_uint32) for f in IN_FIELDS]


class WpOut(ctypes.Structure):
    _fields_ = [(f, ctypes.c_uint32) for f in OUT_FIELDS] + [("seg_map", ctypes.c_uint16 * 256)]


@pytest.fixture(scope="module")
def wp():
    L = ctypes.CDLL(os.path.join(BUILD, "libwalk_plan_harness.so"))
    L.wp_plan.restype = None
    L.wp_plan.argtypes = [ctypes.POINTER(WpIn), ctypes.c_uint64, ctypes.POINTER(WpOut)]
    L.wp_layout.restype = None
    L.wp_layout.argtypes = [ctypes.POINTER(WpIn), ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(WpOut)]
    L.wp_seg_pick.restype = ctypes.c_uint32
    L.wp_seg_pick.argtypes = [ctypes.POINTER(WpIn), ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint32)]
    L.wp_crec_ok.restype = ctypes.c_uint32
    L.wp_crec_ok.argtypes = [ctypes.POINTER(WpIn), ctypes.c_uint32]
    return L


def as_dict(o):
    d = {f: getattr(o, f) for f in OUT_FIELDS}
    d["seg_map"] = list(o.seg_map[:o.seg_map_n])
    return d


# ------------------------------------------------------------------ the model
K_SEG_LAUNCH_MAX, K_AUTO_SEG_EVENTS, K_FOLD3_MAX_SEQ = 32, 32768, 0x7BFF
K_PASS = {1: 1.0, 2: 1.15, 4: 1.28, 8: 1.7, 12: 2.1}


def m_walk_grid(e, cpw_hint):
    nc = e["ncols"]
    cpw = cpw_hint if cpw_hint else (1 if nc <= 256 else 2 if nc <= 512 else 4)
    slices = (nc + cpw - 1) // cpw
    return slices if cpw == 12 else (slices + 7) // 8 * 8


def m_seg_pick(e, n):
    w8 = e["pack16"] and e["max_seq"] <= 0xFFFF and e["B"] <= e["V"]
    best_g, best, cpw = 0, np.float32(1.0), 0
    for c in (1, 2, 4, 8, 12):
        if (e["cpw"] and c != e["cpw"]) or (c >= 8 and not w8):
            continue
        G = min(e["n_cus"] // m_walk_grid(e, c), K_SEG_LAUNCH_MAX)
        while G >= 2 and n < G * K_AUTO_SEG_EVENTS:
            G -= 1
        if G >= 2 and np.float32(K_PASS[c]) / np.float32(G) < best:
            best, best_g, cpw = np.float32(K_PASS[c]) / np.float32(G), G, c
    return best_g, cpw


def m_auto_segments(e, n):
    if not e["seg_auto"] or e["sharded"] or e["rowseg"] or e["segments"] > 1 or not e["ncols"]:
        return 0, 0
    return m_seg_pick(e, n)


def m_index_args(e):
    """add_batch_dev: the launcher's inputs"""
    a = {"ncols": e["ncols"], "mask": e["B"] > e["V"], "cpw_hint": e["cpw"], "cmap": bool(e["sharded"]),
         "crec": bool(e["crec"]), "seg_xmap": bool(e["seg_xmap"]), "seg_g": 0}
    a["pack16"] = bool(e["pack16"]) and e["max_seq"] <= 0xFFFF
    a["fold3"] = a["pack16"] and bool(e["fold3"]) and e["max_seq"] <= K_FOLD3_MAX_SEQ
    if a["cpw_hint"] >= 8 and (not a["pack16"] or a["mask"]):
        a["cpw_hint"] = 4
    return a


def m_seg_xmap(G, n_slices, sgrid):
    xl = [[] for _ in range(8)]

    def put(k, s0, cnt):
        x = 0
        for y in range(1, 8):
            if len(xl[y]) < len(xl[x]):
                x = y
        xl[x].extend(k << 8 | s for s in range(s0, s0 + cnt))

    for k in range(G):
        for s0 in range(0, n_slices - 7, 8):
            put(k, s0, 8)
    if n_slices % 8:
        for k in range(G):
            put(k, n_slices // 8 * 8, n_slices % 8)
    mx = max(len(l) for l in xl)
    if 8 * mx <= 256 and 8 * mx <= sgrid + 8:
        return [xl[g % 8][g // 8] if g // 8 < len(xl[g % 8]) else 0xFFFF for g in range(8 * mx)]
    return []


def m_launch(a):
    """launch_index + launch_index_t: the kernel and its grid"""
    cpw = a["cpw_hint"] if a["cpw_hint"] else (1 if a["ncols"] <= 256 else 2 if a["ncols"] <= 512 else 4)
    if cpw <= 1:
        CPW, NCW, ND = 1, 8, 4
    elif cpw <= 2:
        CPW, NCW, ND = 2, 8, 4
    elif cpw == 8:
        CPW, NCW, ND = 8, 8, 7
    elif cpw == 12:
        CPW, NCW, ND = (8, 8, 7) if a["cmap"] else (12, 8, 7)
    else:
        CPW, NCW, ND = 4, 11, 4
    n_slices = (a["ncols"] + CPW - 1) // CPW
    spx = (n_slices + 7) // 8
    grid = spx * 8
    k = {"cpw": CPW, "ncw": NCW, "nd": ND, "n_slices": n_slices, "slices_per_xcd": spx, "grid": grid, "seg_map": [],
         "segs": bool(a["seg_g"])}
    g = a["seg_g"]
    if CPW >= 8:
        assert a["pack16"] and not a["mask"]   # (the launcher's hipErrorInvalidValue)
        sgrid = 8 * (g * (n_slices // 8) + (g * (n_slices % 8) + 7) // 8) if CPW == 12 else grid * g
        if CPW == 12 and g and a["seg_xmap"] and n_slices <= 255:
            k["seg_map"] = m_seg_xmap(g, n_slices, sgrid)
            if k["seg_map"]:
                sgrid = len(k["seg_map"])
        k.update(masked=False, packed=True, crec=a["crec"], fold3=not a["crec"] and a["fold3"], seg_grid=sgrid)
    else:
        k.update(masked=a["mask"], packed=CPW == 4 and a["pack16"], crec=False, fold3=False, seg_grid=grid * g)
    return k


def m_seg_walk(e, a, G, cpw):
    a = dict(a)
    a["cpw_hint"] = 4 if cpw >= 8 and (not a["pack16"] or a["mask"]) else cpw
    conc = G <= K_SEG_LAUNCH_MAX and G * m_walk_grid(e, a["cpw_hint"]) <= e["n_cus"]
    a["seg_g"] = G if conc else 0
    return a, G, conc


def m_plan(e, n):
    """add_batch_dev's walk of a batch of n events (the row-segment and the
    frontier-doubling paths aside)"""
    a = m_index_args(e)
    G, conc = 0, False
    if e["segments"] > 1 and not e["sharded"] and n >= 64 * e["segments"]:
        a, G, conc = m_seg_walk(e, a, e["segments"], e["cpw"])
    else:
        g, cpw = m_auto_segments(e, n)
        if g:
            a, G, conc = m_seg_walk(e, a, g, cpw)
    return m_finish(e, a, G, conc)


def m_finish(e, a, G, conc):
    k = m_launch(a)
    # no walk_grid call is reachable on a column shard (shards never take the
    # segment paths): the CUs-held figure is compared on whole handles only
    walk_cus = None if e["sharded"] else m_walk_grid(e, a["cpw_hint"])
    return {"cpw": k["cpw"], "ncw": k["ncw"], "nd": k["nd"], "masked": int(k["masked"]), "packed": int(k["packed"]),
            "crec": int(k["crec"]), "fold3": int(k["fold3"]), "n_slices": k["n_slices"],
            "slices_per_xcd": k["slices_per_xcd"], "grid": k["grid"], "walk_cus": walk_cus, "G": G,
            "one_launch": int(conc), "seg_grid": k["seg_grid"], "seg_map_n": len(k["seg_map"]), "seg_map": k["seg_map"]}


def m_layout(e, cpw, G):
    """seg_walk / rs_begin: a walk at a requested width as G segments"""
    a = m_index_args(e)
    if G < 2:
        a["cpw_hint"] = 4 if cpw >= 8 and (not a["pack16"] or a["mask"]) else cpw
        return m_finish(e, a, 0, False)
    a, G, conc = m_seg_walk(e, a, G, cpw)
    return m_finish(e, a, G, conc)


def same(got, exp):
    return all(got[f] == exp[f] for f in exp if exp[f] is not None)


# ------------------------------------------------------------------ the grid
AXES = {
    "ncols": [1, 2, 8, 12, 13, 25, 96, 100, 255, 256, 257, 512, 513, 1000, 1021, 3060, 3061],
    "forks": [0, 1],
    "max_seq": [1, 0x7BFF, 0x7C00, 0xFFFF, 0x10000],
    "cpw": [0, 1, 2, 4, 8, 12],
    "pack16": [0, 1], "fold3": [0, 1], "crec": [0, 1], "seg_xmap": [0, 1], "seg_auto": [0, 1],
    "sharded": [0, 1],
    "segments": [0, 2, 3, 33, 64],
    "n": [63, 64, 128, 32767, 65536, 98304, 1 << 20],
    "n_cus": [64, 256],
}
# the walker's instances (launch_index_t's ladder): cpw, masked, packed, crec, fold3
VARIANTS = ([(c, m, 0, 0, 0) for c in (1, 2, 4) for m in (0, 1)] + [(4, m, 1, 0, 0) for m in (0, 1)] +
            [(c, 0, 1, cr, f3) for c in (8, 12) for cr, f3 in ((0, 0), (1, 0), (0, 1))])
SAMPLE = 12000


def epoch(p):
    e = {f: p.get(f, 0) for f in IN_FIELDS}
    e["V"] = p["ncols"]
    e["B"] = p["ncols"] + (3 if p["forks"] else 0)
    return e


def test_plan_matches_the_model_over_the_grid(wp):
    rng = random.Random(20261020)
    names = list(AXES)
    o = WpOut()
    hit, conc_seen, maps = set(), set(), 0
    for _ in range(SAMPLE):
        p = {k: rng.choice(AXES[k]) for k in names}
        e = epoch(p)
        wp.wp_plan(ctypes.byref(WpIn(**e)), p["n"], ctypes.byref(o))
        got, exp = as_dict(o), m_plan(e, p["n"])
        assert same(got, exp), (p, got, exp)
        hit.add((bool(got["one_launch"]), got["cpw"], got["masked"], got["packed"], got["crec"], got["fold3"]))
        if got["G"]:
            conc_seen.add(got["one_launch"])
        maps += got["seg_map_n"] > 0
    assert len(VARIANTS) == 14
    assert hit == {(s,) + v for s in (False, True) for v in VARIANTS}   # each as k_index and as k_index_segs
    assert conc_seen == {0, 1}
    assert maps > 0


def test_layout_matches_the_model(wp):
    """A requested width as G segments (the option's count, a row-segment
    rank's sub-segments): every width against every segment count."""
    o = WpOut()
    for ncols, forks, max_seq, pack16, crec, n_cus in itertools.product(
            [8, 100, 257, 1000, 1021, 3060], [0, 1], [1, 0x7C00, 0x10000], [0, 1], [0, 1], [64, 256]):
        e = epoch({"ncols": ncols, "forks": forks, "max_seq": max_seq, "pack16": pack16, "fold3": 1, "crec": crec,
                   "seg_xmap": 1, "seg_auto": 1, "n_cus": n_cus})
        for cpw in AXES["cpw"]:
            for G in (0, 1, 2, 3, 7, 32, 33, 64):
                wp.wp_layout(ctypes.byref(WpIn(**e)), cpw, G, ctypes.byref(o))
                got, exp = as_dict(o), m_layout(e, cpw, G)
                assert same(got, exp), (e, cpw, G, got, exp)


def test_seg_pick_matches_the_model(wp):
    c = ctypes.c_uint32()
    for ncols, forks, max_seq, cpw, pack16, n, n_cus in itertools.product(
            AXES["ncols"], [0, 1], [0xFFFF, 0x10000], AXES["cpw"], [0, 1], AXES["n"], AXES["n_cus"]):
        e = epoch({"ncols": ncols, "forks": forks, "max_seq": max_seq, "cpw": cpw, "pack16": pack16, "n_cus": n_cus})
        c.value = 0
        G = wp.wp_seg_pick(ctypes.byref(WpIn(**e)), n, ctypes.byref(c))
        assert (G, c.value if G else 0) == m_seg_pick(e, n), (e, n)


def test_seg_map_properties(wp):
    """What k_index_segs relies on, for every segment count and slice count
    that can get a table: every (walk, slice) pair exactly once, idle entries
    0xFFFF, at most 256 entries -- and the table the model builds."""
    o = WpOut()
    tables = 0
    for n_cus in (256, 1 << 20):   # (the second: the table's own guards, whatever fits the device)
        for n_slices in range(1, 257):
            e = epoch({"ncols": 12 * n_slices, "forks": 0, "max_seq": 1, "cpw": 12, "pack16": 1, "fold3": 1,
                       "seg_xmap": 1, "seg_auto": 1, "n_cus": n_cus})
            for G in range(2, K_SEG_LAUNCH_MAX + 1):
                if n_cus > 256 and 8 * ((G * n_slices + 7) // 8) > 256 + 64:
                    break      # far past the 256 entries: no table for this or any larger G
                wp.wp_layout(ctypes.byref(WpIn(**e)), 12, G, ctypes.byref(o))
                assert o.n_slices == n_slices and o.seg_map_n <= 256
                if not o.seg_map_n:
                    continue
                tables += 1
                m = list(o.seg_map[:o.seg_map_n])
                assert o.one_launch and o.seg_grid == o.seg_map_n and n_slices <= 255
                live = [x for x in m if x != 0xFFFF]
                assert sorted(live) == [k << 8 | s for k in range(G) for s in range(n_slices)]
                assert m == m_seg_xmap(G, n_slices, 8 * (G * (n_slices // 8) + (G * (n_slices % 8) + 7) // 8))
    assert tables > 100


def test_crec_condition(wp):
    """Compact records are written for fork-free epochs whose seqs and
    branches fit 16 bits, under option crec only."""
    for V, forks, max_seq, pack16, opt in itertools.product([100, 0xFFFF, 0x10000], [0, 1], [0xFFFF, 0x10000], [0, 1],
                                                            [0, 1]):
        e = epoch({"ncols": V, "forks": forks, "max_seq": max_seq, "pack16": pack16})
        exp = bool(opt and not forks and pack16 and max_seq <= 0xFFFF and V <= 0xFFFF)
        assert bool(wp.wp_crec_ok(ctypes.byref(WpIn(**e)), opt)) == exp, (e, opt)


def test_anchors(wp):
    """Two plans worked out by hand from the rules."""
    o = WpOut()
    base = {"forks": 0, "max_seq": 1000, "pack16": 1, "fold3": 1, "seg_auto": 1, "n_cus": 256}
    # V = 1000: 12-column slices, 84 of them, three walks side by side in one launch of 256 workgroups
    for n in (98304, 1 << 20, 10_000_000):
        wp.wp_plan(ctypes.byref(WpIn(**epoch(dict(base, ncols=1000)))), n, ctypes.byref(o))
        assert (o.cpw, o.n_slices, o.G, o.one_launch, o.seg_grid) == (12, 84, 3, 1, 256)
        assert (o.ncw, o.nd, o.masked, o.packed, o.crec, o.fold3, o.walk_cus, o.seg_map_n) == (8, 7, 0, 1, 0, 1, 84, 0)
    # V = 100, 100000 events: three segments at width 2
    wp.wp_plan(ctypes.byref(WpIn(**epoch(dict(base, ncols=100)))), 100000, ctypes.byref(o))
    assert (o.cpw, o.G, o.one_launch, o.n_slices, o.grid, o.seg_grid) == (2, 3, 1, 50, 56, 168)
