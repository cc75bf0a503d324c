"""Ancestry on the GPU (include/lachesis_ancestry.h, lachesis_hip.ancestry)
against the CPU model (tests/ancestry_model.py, itself pinned to the oracle by
tests/test_ancestry_model.py), bit for bit: lx_anc_observes over all pairs,
lx_anc_confirm against the reference's walk and the abft oracle's blocks,
rollback, epoch reset, labels handed back after a restart, error paths, and the
calls from inside the abft engine's block callbacks."""

import ctypes

import numpy as np
import pytest

import ancestry_model as am
from abft_harness import topo_shuffle
from oracle import pos, tdag
from oracle.tdag import SplitMix64

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -1, -4
FORKS = (12, 30, 4, 3, 5, 2)
u32p = ctypes.POINTER(ctypes.c_uint32)
u8p = ctypes.POINTER(ctypes.c_uint8)


@pytest.fixture(scope="module")
def lx():
    import lachesis_hip
    return lachesis_hip


def _index(lx, validators, events):
    ix = lx.VecfcIndex()
    ix.reset(validators)
    ix.add_events(events)
    return ix


def _state(anc, m):
    """The whole label table and the low-water mark equal the model's."""
    assert [int(l) for l in anc.labels_dense()] == m.label[:len(anc.dagi.ids)]
    assert anc.low_water() == m.low_water()


def _confirm(anc, m, heads, labels, walk=True):
    """One lx_anc_confirm call against the model: n_new, the events per head
    (ascending), then labels and mark."""
    want = (m.confirm if walk else m.confirm_all_ancestors)(heads, labels)
    got = anc.confirm_dense(heads, labels)                   # cut by n_new
    assert [len(g) for g in got] == [len(w) for w in want]
    for k, (g, w) in enumerate(zip(got, want)):
        assert [int(e) for e in g] == sorted(w), k
    _state(anc, m)
    return got


# ---- lx_anc_observes

@pytest.mark.parametrize("shape", [(1, 6, 1, 0, 0, 1), (4, 6, 3, 0, 0, 2), (7, 25, 3, 0, 0, 1), FORKS,
                                   (9, 20, 3, 9, 4, 7), (257, 3, 8, 5, 2, 6)])
def test_observes_all_pairs(lx, shape):
    """Every (head, x), head = x and x above head included."""
    validators, events = am.build_shape(shape)
    m = am.Model(validators, events)
    anc = lx.AncestryIndex(_index(lx, validators, events))
    n = m.n
    head, x = np.repeat(np.arange(n), n), np.tile(np.arange(n), n)
    got = anc.observes_dense(head, x).reshape(n, n)
    want = m.observes_matrix()
    assert got.diagonal().all() and not np.triu(got, 1).any()
    assert np.array_equal(got, want)
    if shape[3]:                                             # the LowestAfter fallback answered some of them
        _, marked = m.hb_rule_matrix()
        assert want[marked].any()
    ids = [e.id for e in events]                             # by event ID
    assert list(anc.observes([ids[-1], ids[0], ids[-1]], [ids[0], ids[-1], ids[-1]])) == \
        [m.observes(n - 1, 0), n == 1, True]


@pytest.fixture(scope="module")
def wide(lx):
    """1100 validators (rows wider than 1024) with three fork branches."""
    nodes, events = tdag.rand_fork_dag(1100, 3, 4, 3, 1, seed=3)
    validators = pos.Validators(dict(zip(nodes, [1] * 1100)))
    ix = _index(lx, validators, events)
    assert ix.ix.num_branches() > 1100                      # seed 3 holds forks
    return validators, events, ix


def test_observes_wide_rows(lx, wide):
    validators, events, ix = wide
    m = am.Model(validators, events)
    anc = lx.AncestryIndex(ix)
    heads = np.arange(m.n - 64, m.n)
    got = anc.observes_dense(np.repeat(heads, m.n), np.tile(np.arange(m.n), 64)).reshape(64, m.n)
    want = m.observes_matrix()[heads]
    assert np.array_equal(got, want) and want.sum() > 64


def test_confirm_wide_rows(lx, wide):
    """Rows of 1103 branches: 14 heads fit the LDS budget of one launch, so 20
    heads take two; one head alone runs several workgroups."""
    validators, events, ix = wide
    m = am.Model(validators, events)
    anc = lx.AncestryIndex(ix)
    _confirm(anc, m, [1500], [3])
    rng = SplitMix64(21)
    heads = sorted(1500 + rng.below(m.n - 1500) for _ in range(20))
    got = _confirm(anc, m, heads, list(range(10, 30)))
    assert sum(len(g) > 0 for g in got) >= 15


# ---- lx_anc_confirm

@pytest.fixture(scope="module")
def block_cases():
    """shape -> (validators, events, the oracle's blocks), computed once."""
    out = {}
    for shape, min_blocks in am.BLOCK_SHAPES:
        validators, events = am.build_shape(shape)
        blocks = am.oracle_blocks(validators, events)
        assert len(blocks) >= min_blocks
        out[shape] = (validators, events, blocks)
    return out


@pytest.mark.parametrize("one_call", [False, True])
@pytest.mark.parametrize("shape", [s for s, _ in am.BLOCK_SHAPES])
def test_confirm_blocks(lx, block_cases, shape, one_call):
    """Each block's Atropos in its own call, or all of them in one."""
    validators, events, blocks = block_cases[shape]
    m = am.Model(validators, events)
    anc = lx.AncestryIndex(_index(lx, validators, events))
    _state(anc, m)
    atropoi, frames = [b[1] for b in blocks], [b[0] for b in blocks]
    if one_call:
        got = _confirm(anc, m, atropoi, frames)
    else:
        got = [_confirm(anc, m, [a], [f])[0] for a, f in zip(atropoi, frames)]
    for g, b in zip(got, blocks):
        assert [int(e) for e in g] == sorted(b[3]) and len(g) > 0
    ids = [e.id for e in events]                             # GetEventConfirmedOn by ID
    assert [int(l) for l in anc.labels(ids[:5])] == m.label[:5]


@pytest.mark.parametrize("descending", [False, True])
def test_confirm_many_heads(lx, descending):
    """40 arbitrary heads in one call (three launches of 16).  Descending, the
    first head takes almost everything and later ones what is left."""
    validators, events = am.build_shape(FORKS)
    m = am.Model(validators, events)
    anc = lx.AncestryIndex(_index(lx, validators, events))
    rng = SplitMix64(40)
    heads = sorted({rng.below(m.n) for _ in range(60)})[:40]
    assert len(heads) == 40
    if descending:
        heads = heads[::-1]
    got = _confirm(anc, m, heads, [k + 1 for k in range(40)])
    if descending:
        assert len(got[0]) > m.n // 2 and any(len(g) == 0 for g in got[1:])
    else:
        assert all(len(g) > 0 for g in got[:3])


def test_confirm_edge_heads(lx):
    """Event 0, the last event, a duplicate, and an empty call."""
    validators, events = am.build_shape(FORKS)
    m = am.Model(validators, events)
    anc = lx.AncestryIndex(_index(lx, validators, events))
    got = _confirm(anc, m, [0, m.n - 1, m.n - 1, 0], [1, 2, 3, 4])
    assert [int(e) for e in got[0]] == [0] and len(got[1]) > 1 and not len(got[2]) and not len(got[3])
    assert anc.confirm_dense([], []) == [] and len(anc.last_confirmed_dense()) == 0
    _state(anc, m)
    # the list call with a short buffer: the count, and the first `cap` events
    anc2 = lx.AncestryIndex(anc.dagi)
    g, = anc2.confirm_dense([m.n - 1], [7])
    out, n = np.zeros(3, dtype=np.uint32), ctypes.c_uint64()
    assert anc2.L.lx_anc_last_confirmed(anc2.h, out.ctypes.data_as(u32p), 3, ctypes.byref(n)) == 0
    assert n.value == len(g) and list(out) == [int(e) for e in g[:3]]


def test_arbitrary_labels(lx):
    """After labels that are not ancestor-closed the call labels every
    unlabelled ancestor, also behind a labelled event (the reference's walk
    would stop there); a label of 0 takes a label away and lowers the mark."""
    validators, events = am.build_shape((7, 25, 3, 0, 0, 1))
    m = am.Model(validators, events)
    anc = lx.AncestryIndex(_index(lx, validators, events))
    head = m.n - 1
    for e in m.parents[head]:
        m.label[e] = 9
        anc.set_labels_dense(e, [9])
    _state(anc, m)
    got = _confirm(anc, m, [head], [5], walk=False)
    assert len(got[0]) > 1
    m.label[3] = m.label[4] = 0
    anc.set_labels_dense(2, [m.label[2], 0, 0])
    _state(anc, m)
    assert anc.low_water() == 3
    anc.set_labels([events[3].id, events[4].id], [6, 6])     # by event ID
    m.label[3] = m.label[4] = 6
    _state(anc, m)


# ---- rollback, reset, restart

def test_rollback(lx):
    validators, events = am.build_shape(FORKS)
    k, n1 = 150, 260
    ix = _index(lx, validators, events[:k])
    anc = lx.AncestryIndex(ix)
    m = am.Model(validators, events[:n1])
    _confirm(anc, m, [100], [1])
    ix.flush()
    ix.add_events(events[k:n1])
    got = _confirm(anc, m, [n1 - 1], [2])                    # a head in the part that is not flushed
    assert any(int(e) >= k for e in got[0]) and any(int(e) < k for e in got[0])
    kept, low = m.label[:k], min(m.low_water(), k)
    ix.drop_not_flushed()
    assert [int(l) for l in anc.labels_dense()] == kept and anc.low_water() == low
    assert len(anc.last_confirmed_dense()) == 0
    # other events at those indices: none of them has a label
    again = topo_shuffle(events[k:], SplitMix64(5))
    assert [e.id for e in again[:n1 - k]] != [e.id for e in events[k:n1]]
    ix.add_events(again)
    order = events[:k] + again
    m2 = am.Model(validators, order)
    m2.label[:k] = kept
    _state(anc, m2)
    assert not any(anc.labels_dense()[k:])
    _confirm(anc, m2, [len(order) - 1, 200], [3, 4])
    ix.drop_not_flushed()                                    # a second rollback to the same flushed count
    assert [int(l) for l in anc.labels_dense()] == kept and anc.low_water() == low


def test_index_reset_leaves_no_labels(lx):
    validators, events = am.build_shape((7, 25, 3, 0, 0, 1))
    ix = _index(lx, validators, events)
    anc = lx.AncestryIndex(ix)
    m = am.Model(validators, events)
    _confirm(anc, m, [m.n - 1], [4])
    assert anc.low_water() > 0
    ix.flush()
    ix.reset(validators)                                     # lx_reset, not lx_anc_reset
    assert anc.low_water() == 0 and len(anc.last_confirmed_dense()) == 0
    v2, ev2 = am.build_shape((4, 6, 3, 0, 0, 2))             # another validator set in the next epoch
    ix.reset(v2)
    ix.add_events(ev2)
    m2 = am.Model(v2, ev2)
    _state(anc, m2)
    _confirm(anc, m2, [m2.n - 1], [1])
    anc.reset()
    assert anc.low_water() == 0 and not any(anc.labels_dense())


def test_set_labels_resumes(lx, block_cases):
    """The labels fetched halfway through a shape's blocks, put into a fresh
    handle over a re-built index: the rest of the blocks end in the same state."""
    validators, events, blocks = block_cases[(10, 40, 4, 3, 6, 9)]
    m = am.Model(validators, events)
    anc = lx.AncestryIndex(_index(lx, validators, events))
    half = len(blocks) // 2
    for frame, atropos, _, _ in blocks[:half]:
        _confirm(anc, m, [atropos], [frame])
    stored = anc.labels_dense().copy()
    assert stored.any() and not stored.all()
    anc2 = lx.AncestryIndex(_index(lx, validators, events))
    anc2.set_labels_dense(0, stored)
    _state(anc2, m)
    m2 = am.Model(validators, events)
    m2.label = list(m.label)
    for frame, atropos, _, confirmed in blocks[half:]:
        _confirm(anc, m, [atropos], [frame])
        got = _confirm(anc2, m2, [atropos], [frame])
        assert [int(e) for e in got[0]] == sorted(confirmed)
    assert np.array_equal(anc.labels_dense(), anc2.labels_dense())


# ---- errors

def test_error_paths(lx):
    validators, events = am.build_shape((7, 25, 3, 0, 0, 1))
    n = len(events)
    ix = _index(lx, validators, events)
    anc = lx.AncestryIndex(ix)
    m = am.Model(validators, events)
    for head, x in (([n], [0]), ([0], [n]), ([0, n + 7], [0, 0])):
        with pytest.raises(lx.LxError) as ei:
            anc.observes_dense(head, x)
        assert ei.value.code == ERR_ARG and "unknown event" in str(ei.value)
    with pytest.raises(lx.LxError) as ei:
        anc.confirm_dense([3, n], [1, 1])
    assert ei.value.code == ERR_ARG and "unknown event" in str(ei.value)
    with pytest.raises(lx.LxError) as ei:
        anc.confirm_dense([3, 4], [1, 0])
    assert ei.value.code == ERR_ARG and "label 0" in str(ei.value)
    with pytest.raises(lx.LxError) as ei:
        anc.labels_dense(n - 1, 2)
    assert ei.value.code == ERR_ARG
    with pytest.raises(lx.LxError) as ei:
        anc.set_labels_dense(n, [1])
    assert ei.value.code == ERR_ARG
    L, one = anc.L, np.array([1], dtype=np.uint32)
    p1, o8 = one.ctypes.data_as(u32p), np.zeros(1, dtype=np.uint8).ctypes.data_as(u8p)
    assert L.lx_anc_observes(anc.h, 1, None, p1, o8) == ERR_ARG
    assert L.lx_anc_observes(anc.h, 1, p1, p1, None) == ERR_ARG
    assert L.lx_anc_confirm(anc.h, 1, p1, None, p1) == ERR_ARG
    assert L.lx_anc_confirm(anc.h, 1, p1, p1, None) == ERR_ARG
    assert L.lx_anc_last_confirmed(anc.h, None, 0, None) == ERR_ARG
    assert L.lx_anc_labels(anc.h, 0, 1, None) == ERR_ARG
    assert L.lx_anc_set_labels(anc.h, 0, 1, None) == ERR_ARG
    assert L.lx_anc_low_water(anc.h, None) == ERR_ARG
    assert "null" in L.lx_anc_last_error(anc.h).decode()
    h = ctypes.c_void_p()
    assert L.lx_anc_create(None, ctypes.byref(h)) == ERR_ARG
    # the refused calls left nothing behind
    _state(anc, m)
    _confirm(anc, m, [n - 1], [2])
    # a column shard holds partial rows
    sh = lx.Index(shard_rank=0, shard_count=2)
    sh.reset(validators.weights)
    assert sh.L.lx_anc_create(sh.h, ctypes.byref(h)) == ERR_STATE


# ---- from the abft engine's callbacks

def test_confirm_in_begin_block(lx):
    """BeginBlock calls lx_anc_confirm(atropos, frame): per block the set of
    that block's apply_event calls, and afterwards the engine's confirmed-on
    table."""
    validators, events = am.build_shape(FORKS)
    cr, sq, off, par = tdag.to_dense(events, validators)
    asked, errors = [], []

    class Lch(lx.abft.DenseLachesis):
        anc = None

        def _begin(self, user, frame, atropos, cheaters, n):
            super()._begin(user, frame, atropos, cheaters, n)
            try:
                asked.append(self.anc.confirm_dense([atropos], [frame])[0])
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
        assert [int(e) for e in got] == sorted(b[4]) and len(got) > 0
    assert np.array_equal(t.anc.labels_dense(), t.confirmed_on(len(events)))
    assert t.anc.labels_dense().any()
