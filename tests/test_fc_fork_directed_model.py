"""The model of the early exit in fork epochs (tests/fc_fork_directed.py) pinned
on the CPU: its answers equal the oracle's on fork DAGs of more than 512
validators, with the oracle's own rows as input, and the inputs chosen for
tests/test_gpu_fc_early_forks.py exercise what that test is for -- queries
decided in round 1, queries that need the whole rows, both answers, every
quorum equality of every round and every way a cheater can count."""

import numpy as np
import pytest

import fc_directed as fd
import fc_fork_directed as ff
from oracle import corc


def oracle_of(d, w):
    o = corc.OracleIndex(w)
    assert o.add_batch(d.creator, d.seq, d.poff, d.par) == -1
    return o


@pytest.mark.parametrize("V,epv,ch,fk,heavy,seed", [(516, 10, 3, 3, True, 21), (516, 10, 5, 2, False, 22),
                                                    (600, 10, 4, 3, False, 23), (600, 8, 40, 2, False, 24)])
def test_model_equals_oracle(V, epv, ch, fk, heavy, seed):
    d = ff.fork_dag(V, epv, ch, fk, heavy, seed)
    w = ff.zipf(V)
    o = oracle_of(d, w)
    hb, la, bc, branch = ff.oracle_planes(o, d, V)
    assert o.num_branches() > V and (hb & ff.MARK).any()
    assert len(ff.cheaters_of(bc, V)) == ch and ff.gate(w, bc)
    qa, qb = ff.queries(d, 20_000, 5_000, seed)
    m = ff.model(hb, la, bc, branch, w, qa, qb)
    want = o.forkless_cause_batch(qa, qb).astype(bool)
    np.testing.assert_array_equal(m["ans"], want)
    assert m["early"].any() and 0.05 < want.mean() < 0.95
    # the running counts end at fc_directed's reference sums
    ev = np.unique(np.concatenate([qa[:40], qb[:40]]))
    sums, early = fd.ref_sums(hb[ev], la[ev], w, bc, branch[ev])
    ia, ib = np.searchsorted(ev, qa[:40]), np.searchsorted(ev, qb[:40])
    assert np.array_equal(m["total"][:40], sums[ia, ib].astype(np.int64))
    assert np.array_equal(m["early"][:40], early[ia, ib])
    # an early stop never contradicts the final count
    Q = m["quorum"]
    for r in range(3):
        stop = (m["rnd"] == r + 1) & ~m["early"]
        c = m["cum"][r][stop]
        assert np.all((c >= Q) | (c + m["rest"][r] < Q))
        assert np.array_equal(c >= Q, m["total"][stop] >= Q)


@pytest.mark.parametrize("name", list(ff.RANDOM_CASES))
def test_random_cases_cover(name):
    """The GPU test's inputs: the gate is open, the model answers as the oracle,
    >= 20 % of the queries stop in round 1, between 5 % and 95 % of the answers
    are true, and >= 1 % of the queries read round 4 where round 4 can hold
    that many: at V = 1000 it is 488 columns with 9 % of the Zipf stake.  At
    V = 516 it is 4 columns with 0.11 % of the stake (V = 600: 88 columns,
    2.3 %), and a query reads it only when its count after 512 columns lies
    within that much below the quorum -- no choice of seed or window puts 1 %
    of a DAG's queries there, so those cases assert that some query does
    (tests/test_gpu_fc_early_forks.py's directed rows cover the round at
    V = 534 on every quorum equality)."""
    d, w, qa, qb = ff.random_case(name)
    V, _, ch, _, heavy, _, _, _ = ff.RANDOM_CASES[name]
    o = oracle_of(d, w)
    hb, la, bc, branch = ff.oracle_planes(o, d, V)
    cheaters = ff.cheaters_of(bc, V)
    assert len(cheaters) == ch and ff.gate(w, bc)
    assert (cheaters.max() < ch) if heavy else (cheaters.min() >= V - ch)
    m = ff.model(hb, la, bc, branch, w, qa, qb)
    want = o.forkless_cause_batch(qa, qb).astype(bool)
    np.testing.assert_array_equal(m["ans"], want)
    r1, r4, true = (m["rnd"] == 1).mean(), (m["rnd"] == 4).mean(), want.mean()
    print("%s: B=%d round1 %.3f round4 %.3f true %.3f early-false %.3f counters %s" %
          (name, len(bc), r1, r4, true, m["early"].mean(), ff.counters(m["rnd"])))
    assert r1 >= 0.20 and 0.05 < true < 0.95
    assert r4 >= 0.01 if V == 1000 else (m["rnd"] == 4).sum() >= 10
    assert ff.counters(m["rnd"])[0] < len(qa)


@pytest.mark.parametrize("name", list(ff.GATE_CASES))
def test_gate_cases(name):
    """The GPU gate test's inputs miss exactly the condition they are named
    after, and between 5 % and 95 % of their answers are true."""
    V, _, ch, _, _, options, n, _ = ff.GATE_CASES[name]
    d, w, qa, qb = ff.gate_case(name)
    o = oracle_of(d, w)
    B = o.num_branches()
    bc = np.concatenate([np.arange(V), np.zeros(B - V, dtype=np.int64)])
    if ch:
        _, _, bc, _ = ff.oracle_planes(o, d, V)
        assert len(ff.cheaters_of(bc, V)) == ch
    epoch_ok = name not in ("V-512", "long-tail", "equal-stakes", "fork-free")
    assert ff.gate(w, bc) == epoch_ok
    if name == "long-tail":
        assert (B + 3) // 4 - V // 4 > 32 and ch <= ff.MAX_CHEATERS
    if name == "V-512":
        assert ff.gate(ff.zipf(516), np.concatenate([np.arange(516), bc[V:]]))     # only V shuts it
    if name == "equal-stakes":
        assert ff.gate(ff.zipf(V), bc)                                            # only the stakes shut it
    assert (name in ff.GATE_OPEN) == (epoch_ok and not options and n >= ff.MIN_QUERIES)
    assert 0.05 < o.forkless_cause_batch(qa, qb).mean() < 0.95


def test_gate_by_hand():
    """Both sides of the epoch's gate conditions on branch tables written by hand."""
    def bc_of(V, cheaters, forks):
        return np.concatenate([np.arange(V), np.repeat(np.arange(cheaters), forks)])
    assert ff.gate(ff.zipf(516), bc_of(516, 1, 1))
    assert not ff.gate(ff.zipf(512), bc_of(512, 1, 1))            # 512 original columns: no round 4
    assert not ff.gate(ff.zipf(515), bc_of(515, 1, 1))            # t0 = 128
    assert ff.gate(ff.zipf(600), bc_of(600, 64, 2))               # a tail of exactly 32 uint4
    assert not ff.gate(ff.zipf(600), bc_of(600, 43, 3))           # 129 fork branches: 33 uint4
    assert ff.gate(ff.zipf(602), bc_of(602, 63, 2)) and not ff.gate(ff.zipf(602), bc_of(602, 64, 2))   # the straddling uint4 counts
    assert not ff.gate(ff.zipf(600), bc_of(600, 65, 1))           # more cheaters than mask bits
    assert not ff.gate(ff.zipf(600), np.arange(600))              # fork-free
    assert not ff.gate(np.full(1000, 3, dtype=np.uint32), bc_of(1000, 3, 2))   # 512 of 1000 equal stakes < 2/3


def test_rounds_by_hand():
    """The model on rows small enough to follow: V = 520, unit stakes but 400 on
    validator 0 (total 919, quorum 613: columns < 512 reach it), cheaters 1
    (round 1) and 515 (round 4) with one fork branch each (columns 520, 521)."""
    V = 520
    w = np.ones(V, dtype=np.uint32)
    w[0] = 400
    bc = np.concatenate([np.arange(V), [1, 515]])
    assert ff.gate(w, bc) and fd.quorum_of(w) == 613
    assert ff.rests(w) == [392, 264, 8, 0]
    assert [len(c) for c in ff.round_columns(V, len(bc))] == [130, 128, 256, 8]
    hb = np.full((2, 522), 9, dtype=np.uint32)
    hb[1, [515, 521]] |= ff.MARK                   # cheater 515 marked in row 1
    la = np.zeros((6, 522), dtype=np.uint32)
    la[0, :] = 1             # 400 + 127 + [515 through 521] = 528, 656: true in round 2
    la[1, 1:] = 1            # 128 (127 + cheater 515), 256, 512, 519 < 613: 128 + 392 < 613: false in round 1
    la[2, :300] = 1          # 527, 655: true in round 2
    la[3, [0, 515, 521]] = 1     # 401 + 392 >= 613 open, 401 + 264 >= 613 open, 401 + 8 < 613: false in round 3
    la[4, :100] = 1
    la[4, 128:341] = 1       # 499, 627: true in round 2
    la[5, :100] = 1
    la[5, 300:] = 1          # 498 + cheaters 1 and 515 (branches 520, 521) = 500, 500 (+ 264: open), 712: true in round 3
    branch = np.array([0, 515, 2, 3, 521, 5])      # events 1 and 4 sit on cheater 515's branches
    qa = np.array([0] * 6 + [1] * 6)
    qb = np.array(list(range(6)) * 2)
    m = ff.model(hb, la, bc, branch, w, qa, qb)
    assert m["cum"][:, 0].tolist() == [528, 656, 912, 919]
    assert m["rnd"][:6].tolist() == [2, 1, 2, 3, 2, 3]
    assert m["ans"][:6].tolist() == [True, False, True, False, True, True]
    assert m["total"][:6].tolist() == [919, 519, 699, 401, 712, 719]
    # row 1 of hb: cheater 515 counts 0; b = 1 and b = 4 are its events: early false after round 1
    assert m["early"].tolist() == [False] * 6 + [False, True, False, False, True, False]
    assert m["cum"][:, 6].tolist() == [527, 655, 911, 918]
    assert m["rnd"][6:].tolist() == [2, 1, 2, 3, 1, 3]
    assert m["ans"][6:].tolist() == [True, False, True, False, False, True]
    assert ff.counters(m["rnd"]) == (9, 4, 12, 0)


@pytest.fixture(scope="module")
def directed():
    d = ff.directed_dag()
    w = ff.directed_weights()
    o = oracle_of(d, w)
    _, _, bc, branch = ff.oracle_planes(o, d, ff.DIRECTED_V)
    return d, w, bc, branch


def test_directed_rows_reach_every_cell(directed):
    d, w, bc, branch = directed
    V, B, Q = len(w), len(bc), fd.quorum_of(w)
    assert ff.gate(w, bc) and V % 4 and B % 4          # a straddling uint4, pad columns inside the last one read
    ev = ff.directed_events(branch, bc)
    assert len(ev) == ff.N_DIRECTED == len(set(ev.tolist()))
    hb, la, where = ff.directed_case(bc, seed=1)
    N = ff.N_DIRECTED
    E = len(d)
    # the model indexes rows by event: place the rows at their events
    hbe = np.zeros((E, B), dtype=np.uint32)
    lae = np.zeros((E, B), dtype=np.uint32)
    hbe[ev], lae[ev] = hb, la
    qa, qb = np.repeat(ev, N), np.tile(ev, N)
    m = ff.model(hbe, lae, bc, branch, w, qa, qb)
    rnd, cum, rest = m["rnd"].reshape(N, N), m["cum"].reshape(4, N, N), m["rest"]
    ans, early, total = m["ans"].reshape(N, N), m["early"].reshape(N, N), m["total"].reshape(N, N)
    cells = {(r, c) for r in (1, 2, 3, 4) for c in fd.EARLY_CELLS if not (r == 4 and c.startswith("r"))}
    assert cells <= set(where)
    on_cell = lambda c, r, cell: {"q": c == Q, "q-1": c == Q - 1, "r=q": c + rest[r - 1] == Q,
                                  "r=q-1": c + rest[r - 1] == Q - 1}[cell]
    full = [i for i in range(len(fd.FULL_HB)) if not early[i].any()]
    assert len(full) >= 6
    for (r, cell) in sorted(cells):
        k = where[(r, cell)]
        for i in full:
            assert rnd[i, k] >= r and on_cell(int(cum[r - 1, i, k]), r, cell), (r, cell, i)
    ch = np.array(ff.DIRECTED_CHEATERS)
    n_full = len(fd.FULL_HB)
    for name, (r, cell), ci, which in ff.CHEATER_ROWS:
        k = where[name]
        for i in full:
            assert rnd[i, k] >= r and on_cell(int(cum[r - 1, i, k]), r, cell), (name, i)
        # the HB row that marks this cheater: it counts 0 there, the count is its stake short
        i = n_full + ci
        for rr in range(4):
            assert cum[rr, i, k] <= cum[rr, full[0], k]
        assert total[i, k] == total[full[0], k] - int(w[ch[ci]])
    # every round stops queries with either answer, the early false apart
    for r in (1, 2, 3, 4):
        sel = (rnd == r) & ~early
        assert (ans & sel).any() and (~ans & sel).any(), r
    # the early false over a count that reaches the quorum, and one below it
    assert (early & (total >= Q)).any() and (early & (total < Q)).any()
    assert np.all(rnd[early] == 1) and not ans[early].any()
    print("directed: B=%d quorum=%d counters %s early-false %d" % (B, Q, ff.counters(rnd.reshape(-1)), int(early.sum())))
