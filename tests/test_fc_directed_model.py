"""The directed ForklessCause tests' reference (tests/fc_directed.py) pinned on
the CPU: ref_sums answers every pair of a fork-free and of a fork DAG as the
oracle does, and the row constructor reaches every quorum equality it is used
for in tests/test_gpu_fc_directed.py."""

import numpy as np
import pytest

import fc_directed as fd
from oracle import corc

MAX_INT32 = 0x7FFFFFFF


def planes_of(o, d, V):
    """The oracle's rows in plane form: hb[N, B] (a fork marker {0, MaxInt32}
    becomes bit 31 on every branch of that creator), la[N, B], and the branch
    tables (creator of each branch, branch of each event)."""
    N = len(d)
    B = o.num_branches()
    ev = np.arange(N, dtype=np.uint32)
    branch = np.array([o.branch(i) for i in range(N)], dtype=np.int64)
    bc = np.full(B, -1, dtype=np.int64)
    bc[branch] = d.creator
    assert np.all(bc >= 0) and np.array_equal(bc[:V], np.arange(V))
    hb = np.zeros((N, B), dtype=np.uint32)
    la = np.zeros((N, B), dtype=np.uint32)
    off, buf = o.rows(0, ev)
    for i in range(N):
        r = np.frombuffer(buf[int(off[i]):int(off[i + 1])].tobytes(), dtype=np.uint32).reshape(-1, 2)
        hb[i, :len(r)] = r[:, 0]
        marked = np.unique(bc[:len(r)][(r[:, 0] == 0) & (r[:, 1] == MAX_INT32)])
        hb[i, np.isin(bc, marked)] |= fd.MARK
    off, buf = o.rows(1, ev)
    for i in range(N):
        r = np.frombuffer(buf[int(off[i]):int(off[i + 1])].tobytes(), dtype=np.uint32)
        la[i, :len(r)] = r
    return hb, la, bc, branch


@pytest.mark.parametrize("shape", [(7, 12, 3, 0, 0, 1), (9, 20, 4, 3, 5, 2)], ids=["fork-free", "forks"])
def test_ref_sums_equals_oracle(shape):
    from lachesis_hip import tools
    V, epv, p, ch, fk, seed = shape
    d = tools.gen_dag(V, epv, p, cheaters=ch, forks=fk, seed=seed)
    w = np.array([1, 1, 2, 2, 3, 3, 4, 4, 5][:V], dtype=np.uint32)       # the cheaters (first creators) are light
    o = corc.OracleIndex(w)
    assert o.add_batch(d.creator, d.seq, d.poff, d.par) == -1
    N = len(d)
    hb, la, bc, branch = planes_of(o, d, V)
    assert (o.num_branches() > V) == bool(ch)
    if ch:
        sums, early = fd.ref_sums(hb, la, w, bc, branch)
        assert early.any() and (hb & fd.MARK).any()
    else:
        sums, early = fd.ref_sums(hb, la, w)
        s2, e2 = fd.ref_sums(hb, la, w, bc, branch)          # the fork form agrees on fork-free rows
        assert np.array_equal(sums, s2) and not e2.any()
    a = np.repeat(np.arange(N, dtype=np.uint32), N)
    b = np.tile(np.arange(N, dtype=np.uint32), N)
    want = o.forkless_cause_batch(a, b).reshape(N, N).astype(bool)
    got = ~early & (sums >= fd.quorum_of(w))
    np.testing.assert_array_equal(got, want)
    assert 0.05 < want.mean() < 0.95


@pytest.mark.parametrize("L", [32, 16])
@pytest.mark.parametrize("V", [513, 516, 1000, 1025, 1100, 1500])
def test_constructor_hits_every_target(V, L):
    """edge_weights / subset_with_weight: every block reaches every integer, the
    early path's gate is open, and every (round, cell) target exists and the
    rows built for it land on it."""
    w = fd.edge_weights(V, L)
    Q = fd.quorum_of(w)
    blocks = fd.early_blocks(V, L)
    total = int(w.astype(np.uint64).sum())
    assert total < 1 << 31
    assert int(w[:blocks[2][1]].astype(np.uint64).sum()) >= Q
    for lo, hi in blocks:
        W = int(w[lo:hi].astype(np.uint64).sum())
        for t in {0, W // 3, W // 2, W - 1, W} | set(range(min(W, 40))):
            cols = fd.subset_with_weight(w, lo, hi, t)
            assert cols is not None and int(w[cols].sum()) == t and np.all((cols >= lo) & (cols < hi)), (lo, hi, t)
    assert fd.subset_with_weight(w, 0, V, total + 1) is None
    targets = fd.early_targets(w, L)
    assert set(targets) == {(r, c) for r in (1, 2, 3, 4) for c in fd.EARLY_CELLS if not (r == 4 and c.startswith("r"))}
    # the targets the rounds are named after: s1 == quorum, s1 + rest1 ==
    # quorum - 1, an open s1 with s1 + s2 == quorum / s1 + s2 + rest2 == quorum - 1
    W = [int(w[lo:hi].astype(np.uint64).sum()) for lo, hi in blocks]
    assert targets[(1, "q")][0] == Q and targets[(1, "r=q-1")][0] + sum(W[1:]) == Q - 1
    for cell, v in (("q", Q), ("r=q-1", Q - 1 - W[2] - W[3])):
        t = targets[(2, cell)]
        assert t[0] < Q <= t[0] + sum(W[1:]) and t[0] + t[1] == v
    hb, la, where = fd.early_rows(w, L, 256, seed=V)
    rnd, cum, rest, gate = fd.early_model(hb, la, w, Q, L)
    assert gate and rest[3] == 0
    sums, _ = fd.ref_sums(hb, la, w)
    assert np.array_equal(cum[3], sums)
    for (r, cell), k in where.items():
        for i in range(len(fd.FULL_HB)):                     # every full HB row against the target row
            c, rs = int(cum[r - 1, i, k]), rest[r - 1]
            assert rnd[i, k] >= r
            assert {"q": c == Q, "q-1": c == Q - 1, "r=q": c + rs == Q, "r=q-1": c + rs == Q - 1}[cell], (r, cell, i)
    cells = fd.early_cells(rnd, cum, rest, Q)
    assert all(n >= len(fd.FULL_HB) for n in cells.values()), cells
    ans = sums >= Q
    for r in (1, 2, 3, 4):
        assert (ans & (rnd == r)).any() and (~ans & (rnd == r)).any(), r


def test_early_model_by_hand():
    """early_model on a row small enough to follow: L = 1 (blocks of 4, 4, 8
    columns and the rest), unit stakes."""
    V = 20
    w = np.ones(V, dtype=np.uint32)
    Q = fd.quorum_of(w)                                       # 14
    assert Q == 14
    hb = np.full((1, V), 9, dtype=np.uint32)
    la = np.zeros((4, V), dtype=np.uint32)
    la[0, :] = 1                  # 4, 8, 16: decided true in round 3
    la[1, 4:] = 10                # la > hb: nothing counts; 0 + 16 >= 14 open, 0 + 12 < 14: false in round 2
    la[2, :14] = 9                # la == hb counts: 4, 8, 14: true in round 3
    la[3, 2:16] = 1
    la[3, 15] = 0                 # 2, 6, 13 (13 + 4 >= 14: open), 13: false in round 4
    rnd, cum, rest, gate = fd.early_model(hb, la, w, Q, 1)
    assert rest == [16, 12, 4, 0] and gate
    assert rnd[0].tolist() == [3, 2, 3, 4]
    assert cum[:, 0, 3].tolist() == [2, 6, 13, 13]
    sums, early = fd.ref_sums(hb, la, w)
    assert sums[0].tolist() == [20, 0, 14, 13] and not early.any()
