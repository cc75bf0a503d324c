"""The ForklessCause kernels on crafted rows (run on an MI355X: pytest -m gpu).

Random DAGs rarely put a query's stake sum within one light validator of the
quorum, so a kernel that drops or double-counts a column passes them.  Here
the rows are written: a handle indexes a small valid DAG, both planes' rows of
N = 256 events are then overwritten through lx_device_planes with rows built
by tests/fc_directed.py (edge seqs, single columns, subsets exactly on the
quorum, pad columns that would count), and the kernels answer all N x N pairs.
Compared bit-exactly with fc_directed.ref_sums (pinned to the oracle by
tests/test_fc_directed_model.py): the stake sums themselves
(lx_forkless_cause_partial_dev), the booleans, and the early exit's per-round
query counts.  Nothing is added, flushed or dropped after the overwrite.
"""

import ctypes

import numpy as np
import pytest

import fc_directed as fd

pytestmark = pytest.mark.gpu

N = 256
A = np.repeat(np.arange(N, dtype=np.uint32), N)
B = np.tile(np.arange(N, dtype=np.uint32), N)


@pytest.fixture(scope="module")
def lx():
    import lachesis_hip
    return lachesis_hip


def chain_dag(V, n):
    """n events, creator i % V, each with its self-parent only."""
    i = np.arange(n, dtype=np.int64)
    creator = (i % V).astype(np.uint32)
    seq = (i // V + 1).astype(np.uint32)
    has = i >= V
    poff = np.zeros(n + 1, dtype=np.uint64)
    poff[1:] = np.cumsum(has)
    par = (i[has] - V).astype(np.uint32)
    return creator, seq, poff, par if len(par) else np.zeros(1, dtype=np.uint32)


def write_rows(ix, ev, hb, la):
    """Overwrite the HighestBefore and LowestAfter plane rows of events `ev`
    with hb / la ([n, <= stride]; pad columns up to the stride get hb =
    0x7FFFFFFF, la = 1: entries that count wherever a stake meets them)."""
    import torch
    ix.sync()
    p_hb, p_la, stride, _ = ix.device_planes()
    assert hb.shape[1] <= stride and la.shape[1] <= stride
    hip = ctypes.CDLL("libamdhip64.so.7")
    hip.hipMemcpy.restype = ctypes.c_int
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    assert int(max(ev)) < ix.num_events()
    for plane, rows, pad in ((p_hb, hb, 0x7FFFFFFF), (p_la, la, 1)):
        rows = np.ascontiguousarray(fd.pad_rows(rows, stride, pad))
        for k, e in enumerate(ev):
            assert hip.hipMemcpy(plane + int(e) * stride * 4, rows[k].ctypes.data, stride * 4, 1) == 0
    torch.cuda.synchronize()
    return stride


def device_sums(ix, qa, qb):
    """lx_forkless_cause_partial_dev: the stake sum of every query (bit 31:
    the early false of a fork epoch)."""
    import torch
    dev = torch.device("cuda", 0)
    ta = torch.from_numpy(qa.view(np.int32)).to(dev)
    tb = torch.from_numpy(qb.view(np.int32)).to(dev)
    out = torch.full((len(qa),), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ix.forkless_cause_partial_dev(len(qa), ta.data_ptr(), tb.data_ptr(), out.data_ptr())
    ix.sync()
    return out.cpu().numpy().view(np.uint32)


# V at every lane width of launch_fc (2 lanes for <= 2 uint4, 4 <= 16, 8 <= 32,
# 16 <= 64, 32 <= 128, 64 beyond), on both sides of each switch, not multiples
# of 4, and past 1024 columns (k_fc<64>'s loop for rows longer than 4 uint4 per lane)
@pytest.mark.parametrize("V", [1, 2, 3, 5, 8, 9, 64, 65, 128, 129, 256, 257, 512, 513, 1000, 1023, 1024, 1025, 1029,
                               1500, 2100])
def test_whole_row_sums(lx, V):
    """k_fc<LPQ, false>: the sum of every pair equals ref_sums, the booleans
    follow from it, for every stake set of whole_row_weights."""
    ix = lx.Index(options={"fc_early": 0})
    for name, w in fd.whole_row_weights(V, seed=V).items():
        ix.reset(w)
        ix.add_batch(*chain_dag(V, max(N, V)))
        assert ix.num_branches() == V
        Q = fd.quorum_of(w)
        assert ix.quorum() == Q
        hb, la, qrows = fd.whole_rows(w, N, seed=V)
        want, _ = fd.ref_sums(hb, la, w)
        if name == "pow2" or (name == "ones" and V >= 6):
            # rows exactly below, on and (if the total allows) above the quorum
            assert sorted(qrows) == [dl for dl in (-1, 0, 1) if Q + dl <= int(w.sum())]
            for delta, k in qrows.items():
                assert np.all(want[:len(fd.FULL_HB), k] == Q + delta)
        write_rows(ix, np.arange(N), hb, la)
        got = device_sums(ix, A, B).reshape(N, N)
        bad = np.argwhere(got != want)
        assert not len(bad), (name, [(int(i), int(k), int(got[i, k]), int(want[i, k])) for i, k in bad[:5]])
        ans = ix.forkless_cause_batch(A, B).reshape(N, N)
        np.testing.assert_array_equal(ans, (want >= Q).astype(np.uint8), err_msg=name)
        # a launch below 2^14 queries (pinned answers)
        np.testing.assert_array_equal(ix.forkless_cause_batch(A[:5000], B[:5000]), (want >= Q).reshape(-1)[:5000])
        assert ix.fc_early_rounds()[0] == 0
    ix.close()


@pytest.mark.parametrize("L", [32, 16])
@pytest.mark.parametrize("V", [513, 516, 1000, 1025, 1100, 1500])
def test_early_exit_rounds(lx, V, L):
    """k_fc_early<., 32> / <., 16> on rows that sit on every quorum equality in
    every round: the booleans equal the reference and the device's per-round
    counters equal early_model's prediction exactly."""
    w = fd.edge_weights(V, L)
    Q = fd.quorum_of(w)
    hb, la, _ = fd.early_rows(w, L, N, seed=V)
    rnd, cum, rest, gate = fd.early_model(hb, la, w, Q, L)
    want, _ = fd.ref_sums(hb, la, w)
    ans = want >= Q
    # from the reference alone: every cell is populated
    assert gate
    cells = fd.early_cells(rnd, cum, rest, Q)
    assert len(cells) == 14 and all(n > 0 for n in cells.values()), cells
    for r in (1, 2, 3, 4):
        assert (ans & (rnd == r)).any() and (~ans & (rnd == r)).any(), r
    predicted = (N * N, int((rnd >= 2).sum()), int((rnd >= 3).sum()), int((rnd >= 4).sum()))
    print("V=%d L=%d quorum=%d early rounds predicted %s" % (V, L, Q, predicted))

    ix = lx.Index(options={"fc_early_lanes": L})
    ix.reset(w)
    ix.add_batch(*chain_dag(V, V))
    assert ix.quorum() == Q
    write_rows(ix, np.arange(N), hb, la)
    ix.fc_early_rounds()
    got = ix.forkless_cause_batch(A, B).reshape(N, N)
    rounds = ix.fc_early_rounds()
    np.testing.assert_array_equal(got, ans.astype(np.uint8))
    assert rounds == predicted
    # the whole-row kernel on the same rows: the same sums
    np.testing.assert_array_equal(device_sums(ix, A, B).reshape(N, N), want)
    assert ix.fc_early_rounds()[0] == 0
    ix.close()


@pytest.mark.parametrize("L", [32, 16])
def test_early_exit_gate_shut_on_equal_stakes(lx, L):
    """Equal stakes at V = 1000: the first 16L columns cannot reach the quorum,
    so no launch takes the early path (its counter stays 0), and the answers
    on the same crafted rows still equal the reference."""
    V = 1000
    w = np.full(V, 3, dtype=np.uint32)
    Q = fd.quorum_of(w)
    hb, la, _ = fd.whole_rows(w, N, seed=L)
    want, _ = fd.ref_sums(hb, la, w)
    assert not fd.early_model(hb, la, w, Q, L)[3]
    ix = lx.Index(options={"fc_early_lanes": L})
    ix.reset(w)
    ix.add_batch(*chain_dag(V, V))
    write_rows(ix, np.arange(N), hb, la)
    ix.fc_early_rounds()
    got = ix.forkless_cause_batch(A, B).reshape(N, N)
    assert ix.fc_early_rounds()[0] == 0
    np.testing.assert_array_equal(got, (want >= Q).astype(np.uint8))
    ix.close()


FORK_SHAPES = {
    # name: (V, events/validator, parents, cheaters, forks, seed, option fc_fk, (min, max) cheaters)
    "fk-u32": (100, 14, 10, 20, 4, 20, 1, (1, 32)),          # k_fc_fk<., uint32_t>
    "fk-u64": (100, 14, 10, 40, 4, 40, 1, (33, 64)),         # k_fc_fk<., uint64_t>
    "loop": (101, 14, 10, 20, 4, 20, 0, (1, 64)),            # k_fc<., true>: the cheater fix-up loop, V % 4 != 0
    "fk-u32-wide": (1000, 5, 10, 20, 4, 7, 1, (1, 32)),      # B > 1024: k_fc_fk's loop past 4 uint4 per lane
    "fk-u64-wide": (1000, 5, 10, 40, 4, 9, 1, (33, 64)),
    "loop-wide": (1101, 5, 10, 20, 4, 8, 0, (1, 64)),        # V > 1024: k_fc<64, true>'s loop
}


@pytest.mark.parametrize("shape", list(FORK_SHAPES))
def test_fork_kernels_on_crafted_rows(lx, shape):
    """The fork kernels over a real fork DAG's branch tables: sums (bit 31 =
    early false) and booleans equal ref_sums with the per-creator dedupe,
    marked creators and the early false; stakes of which every integer is a
    subset sum, so rows sit exactly on the quorum here too."""
    V, epv, p, ch, fk, seed, fc_fk, (lo, hi) = FORK_SHAPES[shape]
    d = lx.tools.gen_dag(V, epv, p, cheaters=ch, forks=fk, seed=seed)
    w = fd.mixed_radix_weights(V)
    Q = fd.quorum_of(w)
    ix = lx.Index(options={"fc_fk": fc_fk})
    ix.reset(w)
    br = ix.add_batch(d.creator, d.seq, d.poff, d.par, want_branches=True)
    nB = ix.num_branches()
    assert nB > V
    if shape.endswith("wide"):
        assert nB > 1024
    _, bc = ix.branches_info()
    assert len(bc) == nB and lo <= int((np.bincount(bc, minlength=V) >= 2).sum()) <= hi
    # the rows of N events: half the first events, half events of fork branches
    forked = np.flatnonzero(br >= V)[:N // 2]
    ev = np.concatenate([np.setdiff1d(np.arange(len(d)), forked)[:N - len(forked)], forked]).astype(np.uint32)
    assert len(ev) == N and len(forked) >= 40
    assert [ix.branch(int(e)) for e in ev[::17]] == [int(br[e]) for e in ev[::17]]
    hb, la, qrows = fd.fork_rows(bc, w, N, seed=seed)
    want, early = fd.ref_sums(hb, la, w, bc, br[ev])
    assert sorted(qrows) == [-1, 0, 1]                       # rows exactly below, on and above the quorum
    for delta, k in qrows.items():
        assert np.all(want[:len(fd.FULL_HB), k] == Q + delta)
    assert early.any() and 0.05 < (~early & (want >= Q)).mean() < 0.95
    write_rows(ix, ev, hb, la)
    got = device_sums(ix, ev[A], ev[B]).reshape(N, N)
    want32 = (want + early.astype(np.uint64) * fd.MARK).astype(np.uint32)
    bad = np.argwhere(got != want32)
    assert not len(bad), [(int(i), int(k), hex(got[i, k]), hex(want32[i, k])) for i, k in bad[:5]]
    ans = ix.forkless_cause_batch(ev[A], ev[B]).reshape(N, N)
    np.testing.assert_array_equal(ans, (~early & (want >= Q)).astype(np.uint8))
    ix.close()
