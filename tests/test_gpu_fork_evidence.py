"""Fork evidence on the GPU (lx_anc_fork_pairs / lx_anc_cheaters of
include/lachesis_ancestry.h, lachesis_hip.ancestry) against the CPU model
(tests/fork_evidence_model.py, itself pinned to the oracle's fork markers by
tests/test_fork_evidence_model.py), bit for bit: every (head, creator) of the
seeded fork shapes, the hand-built DAGs, rows wider than 1024, the cheater
lists, the calls from inside the abft engine's begin_block, rollback, epoch
reset, a reload of persisted tables, and the error paths."""

import ctypes

import numpy as np
import pytest

import ancestry_model as am
import fork_evidence_dags as fd
import fork_evidence_model as fm
from abft_harness import topo_shuffle
from oracle import pos, tdag
from oracle.tdag import SplitMix64

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -1, -4
FORKS = (12, 30, 4, 3, 5, 2)
FORK_SHAPES = [s for s in am.PAIR_SHAPES if s[3]]
u32p = ctypes.POINTER(ctypes.c_uint32)


@pytest.fixture(scope="module")
def lx():
    import lachesis_hip
    return lachesis_hip


def _index(lx, validators, events):
    ix = lx.VecfcIndex()
    ix.reset(validators)
    ix.add_events(events)
    return ix


def _all_pairs(anc, m, heads=None):
    """Every (head, creator) of ``heads`` (default: all events) equals the
    model; returns the number of pairs with evidence."""
    heads = np.arange(m.n) if heads is None else np.asarray(heads)
    V = len(m.validators.weights)
    h, c = np.repeat(heads, V), np.tile(np.arange(V), len(heads))
    x, y, s = anc.fork_pairs_dense(h, c)
    wx, wy, ws = fm.evidence_all(m, heads)
    assert np.array_equal(x.reshape(-1, V), wx)
    assert np.array_equal(y.reshape(-1, V), wy)
    assert np.array_equal(s.reshape(-1, V), ws)
    # whatever the tie-break: two different events of that creator with that seq, both observed by the head
    has = x != fm.NONE
    assert np.array_equal(has, y != fm.NONE) and not s[~has].any()
    cr, sq = np.asarray(m.creator), np.asarray(m.seq)
    hx, hy = x[has], y[has]
    assert (hx != hy).all() and (cr[hx] == c[has]).all() and (cr[hy] == c[has]).all()
    assert (sq[hx] == s[has]).all() and (sq[hy] == s[has]).all()
    assert anc.observes_dense(h[has], hx).all() and anc.observes_dense(h[has], hy).all()
    return int(has.sum())


def _cheaters(anc, m, heads):
    got = anc.cheaters_dense(heads)
    assert got == [fm.cheaters(m, h) for h in heads]
    return got


# ---- lx_anc_fork_pairs

@pytest.mark.parametrize("shape", FORK_SHAPES)
def test_fork_pairs_all_pairs(lx, shape):
    validators, events = am.build_shape(shape)
    m = am.Model(validators, events)
    anc = lx.AncestryIndex(_index(lx, validators, events))
    assert _all_pairs(anc, m) > 500
    ids = [e.id for e in events]                             # by event ID
    want = fm.evidence_row(m, m.n - 1)
    c = min(want)
    a, b, s = want[c]
    assert anc.fork_pairs([ids[-1], ids[0]], [c, c]) == [(ids[a], ids[b], s), None]
    assert anc.cheaters([ids[-1]]) == [[(k, ids[p], ids[q], t) for k, (p, q, t) in sorted(want.items())]]


@pytest.mark.parametrize("name", list(fd.DAGS))
def test_directed_dags(lx, name):
    d = fd.DAGS[name]()
    anc = lx.AncestryIndex(_index(lx, d.validators, d.events))
    heads, creators = [h for h, _, _ in d.cases], [c for _, c, _ in d.cases]
    x, y, s = anc.fork_pairs_dense(heads, creators)
    assert [(int(a), int(b), int(q)) for a, b, q in zip(x, y, s)] == [w for _, _, w in d.cases]
    m = am.Model(d.validators, d.events)
    _all_pairs(anc, m)
    _cheaters(anc, m, sorted(set(heads)))
    if name == "many":
        assert anc.dagi.ix.num_branches() == d.V + fd.MANY - 1


def test_fork_pairs_wide_rows(lx):
    """1100 validators (rows wider than 1024) with three fork branches."""
    nodes, events = tdag.rand_fork_dag(1100, 3, 4, 3, 1, seed=3)
    validators = pos.Validators(dict(zip(nodes, [1] * 1100)))
    ix = _index(lx, validators, events)
    assert ix.ix.num_branches() > 1100
    m = am.Model(validators, events)
    anc = lx.AncestryIndex(ix)
    heads = list(range(2 * 1100, m.n))                       # every event of the last round x 1100 creators
    assert _all_pairs(anc, m, heads) == 21
    assert [len(g) for g in _cheaters(anc, m, [2234, 3288, m.n - 1])] == [1, 1, 0]


def test_fork_free_shape_answers_none(lx):
    validators, events = am.build_shape((7, 25, 3, 0, 0, 1))
    m = am.Model(validators, events)
    anc = lx.AncestryIndex(_index(lx, validators, events))
    assert _all_pairs(anc, m) == 0
    assert _cheaters(anc, m, [0, m.n - 1]) == [[], []]
    x, y, c = (np.zeros(1, dtype=np.uint32) for _ in range(3))
    one = np.array([m.n - 1], dtype=np.uint32)
    assert anc.L.lx_anc_fork_pairs(anc.h, 1, one.ctypes.data_as(u32p), c.ctypes.data_as(u32p), x.ctypes.data_as(u32p),
                                   y.ctypes.data_as(u32p), None) == 0   # out_seq is optional
    assert (int(x[0]), int(y[0])) == (fm.NONE, fm.NONE)


# ---- lx_anc_cheaters

def test_cheaters_lists(lx):
    """1 head, 40 heads, a duplicate head, an empty call, the short fetch."""
    validators, events = am.build_shape(FORKS)
    m = am.Model(validators, events)
    anc = lx.AncestryIndex(_index(lx, validators, events))
    got = _cheaters(anc, m, [m.n - 1])
    assert len(got[0]) == 3
    rng = SplitMix64(40)
    heads = sorted({rng.below(m.n) for _ in range(60)})[:40][::-1]
    assert len(heads) == 40
    got = _cheaters(anc, m, heads)
    assert any(len(g) == 0 for g in got) and sum(len(g) for g in got) > 40
    got = _cheaters(anc, m, [m.n - 1, 0, m.n - 1])
    assert got[0] == got[2] and got[0] and not got[1]
    # the list call with a short buffer: the count, and the first `cap` entries
    want = got[0] + got[2]
    c, x, y = (np.zeros(4, dtype=np.uint32) for _ in range(3))
    n = ctypes.c_uint64()
    assert anc.L.lx_anc_last_cheaters(anc.h, c.ctypes.data_as(u32p), x.ctypes.data_as(u32p), y.ctypes.data_as(u32p),
                                      None, 4, ctypes.byref(n)) == 0
    assert n.value == len(want) == 6
    assert [(int(a), int(b), int(d)) for a, b, d in zip(c, x, y)] == [w[:3] for w in want[:4]]
    assert anc.cheaters_dense([]) == [] and len(anc.last_cheaters_dense()[0]) == 0
    # the other calls of the handle neither read nor change any of this
    anc.confirm_dense([m.n - 1], [5])
    _cheaters(anc, m, [m.n - 1])
    assert anc.low_water() > 0


def test_cheaters_more_queries_than_one_launch(lx):
    """252,000 heads x 9 cheaters: three launches of at most 2^20 (head,
    cheater) queries; the second continues a list that has to grow."""
    validators, events = am.build_shape((9, 20, 3, 9, 4, 7))
    m = am.Model(validators, events)
    anc = lx.AncestryIndex(_index(lx, validators, events))
    reps = 1400
    assert m.n * reps * 9 > 2 << 20
    heads = np.tile(np.arange(m.n, dtype=np.uint32), reps)
    per_head = [fm.cheaters(m, h) for h in range(m.n)]
    n_found = np.zeros(len(heads), dtype=np.uint32)
    assert anc.L.lx_anc_cheaters(anc.h, len(heads), heads.ctypes.data_as(u32p), n_found.ctypes.data_as(u32p)) == 0
    assert np.array_equal(n_found, np.tile([len(g) for g in per_head], reps))
    once = np.array([t for g in per_head for t in g], dtype=np.uint32)
    assert len(once) == 1364
    got = np.stack(anc.last_cheaters_dense(), axis=1)
    assert np.array_equal(got, np.tile(once, (reps, 1)))


def test_cheaters_in_begin_block(lx):
    """BeginBlock asks lx_anc_cheaters(atropos): per block the creators are the
    block's cheaters argument, with the model's pairs."""
    validators, events = am.build_shape(FORKS)
    m = am.Model(validators, events)
    cr, sq, off, par = tdag.to_dense(events, validators)
    asked, errors = [], []

    class Lch(lx.abft.DenseLachesis):
        anc = None

        def _begin(self, user, frame, atropos, cheaters, n):
            super()._begin(user, frame, atropos, cheaters, n)
            try:
                asked.append(self.anc.cheaters_dense([atropos])[0])
            except Exception as e:                           # (a callback cannot raise)
                errors.append(e)

    t = Lch(validators.weights)

    class _Dagi:                                             # what AncestryIndex needs of its index
        ix, ids = t.ix, events
    t.anc = lx.ancestry.AncestryIndex(_Dagi)
    rc, consumed, _ = t.process_batch(cr, sq, off, par)
    assert rc == 0 and consumed == len(events) and not errors
    assert len(t.blocks) >= 7 and len(asked) == len(t.blocks)
    for got, b in zip(asked, t.blocks):
        assert [g[0] for g in got] == sorted(int(c) for c in b[3])
        assert got == fm.cheaters(m, b[2])
    assert any(asked)


# ---- rollback, reset, reload

def test_rollback(lx):
    validators, events = am.build_shape((40, 12, 6, 8, 4, 3))
    k, n1 = 42, 200
    ix = _index(lx, validators, events[:k])
    anc = lx.AncestryIndex(ix)
    m = am.Model(validators, events[:n1])
    ix.flush()
    ix.add_events(events[k:n1])
    # evidence whose pair lies in the part that is not flushed
    late = [(h, c) for h in range(k, n1) for c, t in fm.evidence_row(m, h).items() if t[0] >= k]
    assert late
    x, y, _ = anc.fork_pairs_dense([h for h, _ in late], [c for _, c in late])
    assert (x >= k).all() and (y > x).all()
    _all_pairs(anc, m)
    assert any(_cheaters(anc, m, [n1 - 1, late[0][0]]))
    ix.drop_not_flushed()
    assert len(anc.last_cheaters_dense()[0]) == 0
    assert _all_pairs(anc, am.Model(validators, events[:k])) == 0
    # other events at those indices
    again = topo_shuffle(events[k:], SplitMix64(5))
    assert [e.id for e in again[:n1 - k]] != [e.id for e in events[k:n1]]
    ix.add_events(again)
    order = events[:k] + again
    m2 = am.Model(validators, order)
    assert _all_pairs(anc, m2) == 3059
    assert all(_cheaters(anc, m2, [len(order) - 1, 200]))
    ix.drop_not_flushed()
    assert len(anc.last_cheaters_dense()[0]) == 0
    with pytest.raises(lx.LxError) as ei:                    # the dropped indices name no event
        anc.fork_pairs_dense([k], [0])
    assert ei.value.code == ERR_ARG


def test_index_reset_to_another_validator_set(lx):
    validators, events = am.build_shape(FORKS)
    ix = _index(lx, validators, events)
    anc = lx.AncestryIndex(ix)
    m = am.Model(validators, events)
    assert any(_cheaters(anc, m, [m.n - 1]))
    ix.flush()
    ix.reset(validators)                                     # lx_reset, not lx_anc_reset
    assert len(anc.last_cheaters_dense()[0]) == 0
    v2, ev2 = am.build_shape((9, 20, 3, 9, 4, 7))            # every validator of the next epoch forks
    ix.reset(v2)
    ix.add_events(ev2)
    m2 = am.Model(v2, ev2)
    assert _all_pairs(anc, m2) > 500
    with pytest.raises(lx.LxError) as ei:                    # creator 9..11 were validators of the epoch before
        anc.fork_pairs_dense([0], [9])
    assert ei.value.code == ERR_ARG
    assert any(_cheaters(anc, m2, [m2.n - 1]))
    v3, ev3 = am.build_shape((4, 6, 3, 0, 0, 2))             # and a fork-free one
    ix.flush()
    ix.reset(v3)
    ix.add_events(ev3)
    assert _all_pairs(anc, am.Model(v3, ev3)) == 0
    anc.reset()
    assert len(anc.last_cheaters_dense()[0]) == 0


def test_reload_of_a_persisted_epoch(lx):
    """A fresh handle loaded from the written-back tables (lx_load_rows /
    lx_load_finish): LX_ERR_STATE while it loads, the model's answers after."""
    validators, events = am.build_shape(FORKS)
    m = am.Model(validators, events)
    cr, sq, off, par = tdag.to_dense(events, validators)
    A = lx.Index()
    A.reset(validators.weights)
    A.add_batch(cr, sq, off, par)
    wb = A.writeback()
    A.flush()
    N = m.n
    R = lx.Index()
    R.reset(validators.weights)

    class _Dagi:
        ix, ids = R, events
    anc = lx.AncestryIndex(_Dagi)
    R.load_rows(cr, sq, off, par, b"".join(wb["b"][k] for k in range(N)), [wb["S"][k] for k in range(N)],
                [wb["s"][k] for k in range(N)])
    for call in (lambda: anc.fork_pairs_dense([N - 1], [0]), lambda: anc.cheaters_dense([N - 1])):
        with pytest.raises(lx.LxError) as ei:
            call()
        assert ei.value.code == ERR_STATE
    R.load_finish(wb["B"])
    assert _all_pairs(anc, m) == 993
    assert any(_cheaters(anc, m, [N - 1, N // 2]))
    anc.close()
    A.close()
    R.close()


# ---- errors

def test_error_paths(lx):
    validators, events = am.build_shape(FORKS)
    n, V = len(events), 12
    anc = lx.AncestryIndex(_index(lx, validators, events))
    m = am.Model(validators, events)
    before = _cheaters(anc, m, [n - 1])
    for heads, creators, what in (([n], [0], "unknown event"), ([0, n + 7], [0, 0], "unknown event"),
                                  ([0], [V], "unknown creator"), ([0, 1], [1, 0xFFFFFFFF], "unknown creator")):
        with pytest.raises(lx.LxError) as ei:
            anc.fork_pairs_dense(heads, creators)
        assert ei.value.code == ERR_ARG and what in str(ei.value)
    with pytest.raises(lx.LxError) as ei:
        anc.cheaters_dense([3, n])
    assert ei.value.code == ERR_ARG and "unknown event" in str(ei.value)
    L, one = anc.L, np.array([1], dtype=np.uint32)
    p1, n64 = one.ctypes.data_as(u32p), ctypes.c_uint64()
    assert L.lx_anc_fork_pairs(anc.h, 1, None, p1, p1, p1, p1) == ERR_ARG
    assert L.lx_anc_fork_pairs(anc.h, 1, p1, None, p1, p1, p1) == ERR_ARG
    assert L.lx_anc_fork_pairs(anc.h, 1, p1, p1, None, p1, p1) == ERR_ARG
    assert L.lx_anc_fork_pairs(anc.h, 1, p1, p1, p1, None, p1) == ERR_ARG
    assert L.lx_anc_fork_pairs(anc.h, 0, None, None, None, None, None) == 0
    assert L.lx_anc_cheaters(anc.h, 1, None, p1) == ERR_ARG
    assert L.lx_anc_cheaters(anc.h, 1, p1, None) == ERR_ARG
    assert L.lx_anc_last_cheaters(anc.h, p1, p1, p1, p1, 1, None) == ERR_ARG
    assert L.lx_anc_last_cheaters(anc.h, None, p1, p1, p1, 1, ctypes.byref(n64)) == ERR_ARG
    assert L.lx_anc_last_cheaters(anc.h, p1, p1, None, p1, 1, ctypes.byref(n64)) == ERR_ARG
    assert "null" in L.lx_anc_last_error(anc.h).decode()
    assert L.lx_anc_fork_pairs(None, 1, p1, p1, p1, p1, p1) == ERR_ARG
    assert one[0] == 1
    # the refused calls left the last list and everything else as they were
    c, x, y, s = anc.last_cheaters_dense()
    assert [(int(a), int(b), int(d), int(e)) for a, b, d, e in zip(c, x, y, s)] == before[0] and before[0]
    _cheaters(anc, m, [n - 1, 5])
    assert not anc.labels_dense().any() and anc.low_water() == 0
