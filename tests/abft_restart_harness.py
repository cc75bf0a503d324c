"""Helpers shared by the abft restart tests (tests/test_abft_restart_oracle.py
on the CPU, tests/test_gpu_abft_restart.py on the GPU).

``abft/restart_test.go:156-188`` restarts an instance by copying its DBs into
a fresh store, building a new IndexedLachesis with a fresh index over it and
calling Bootstrap.  Here the store is the oracle's ``ao.Store``:

* ``copy_store``       -- the DB copy, optionally with each frame's roots in the
  order the kvdb iterator returns them (key = frame | validator id | event id,
  ``abft/store_roots.go:13-20``) instead of the cache's append order, and
  optionally with the last decided frame rewound (a copy taken before the last
  frames' writes): the confirmed entries above it are dropped with it;
* ``ReplayIndex``      -- the fresh index: the oracle's index keeps no tables to
  reload, so its ``reset`` (called by Bootstrap's epoch-DB-loaded callback,
  ``abft/indexed_lachesis.go:84-99``) re-adds and flushes the persisted events;
* ``store_from_state`` / ``state_from_store`` -- the same copy for a GPU
  instance, whose ``state()`` holds dense indices;
* ``restart_oracle`` / ``restart_gpu`` -- a restarted ``FakeLachesis`` that keeps
  the blocks recorded so far (the application's side of the restart).
"""

import functools

import numpy as np

from oracle import abft_oracle as ao
from oracle import tdag
from oracle.tdag import SplitMix64
from abft_harness import FakeLachesis, node_ids

# (weights, cheaters, events per node, seed): the weight sets of
# abft/restart_test.go:22-64 that differ in shape
RESTART_SHAPES = [
    ([1], 0, 40, 41),
    ([1, 2, 3, 4], 0, 40, 42),
    ([1, 1, 1, 1], 1, 40, 43),
    ([33, 67], 1, 40, 48),
    ([11, 11, 11, 67], 3, 40, 45),
    ([11, 11, 11, 33, 34], 3, 36, 46),
    ([1, 2, 1, 2, 1, 2, 1, 2, 1, 2], 3, 30, 47),
]


def gen_events(weights, cheaters, events_per_node, seed, parent_count=None):
    """As tests/test_gpu_abft.py::gen_events; parentCount = min(5, nodes)
    (restart_test.go:113-116), forks_count = 10."""
    nodes = node_ids(len(weights), seed=seed)
    pc = min(5, len(weights)) if parent_count is None else parent_count
    _, evs = tdag.rand_fork_dag(len(nodes), events_per_node, pc, cheaters=cheaters, forks_count=10,
                                node_ids=nodes, rng=SplitMix64(seed))
    return nodes, evs


class ReplayIndex(ao.DenseOracleIndex):
    """A fresh index over a persisted epoch: the first ``reset`` re-adds and
    flushes ``persisted`` (processing order)."""

    def __init__(self, persisted):
        super().__init__()
        self.persisted = list(persisted)

    def reset(self, validators, get_event=None):
        super().reset(validators, get_event)
        for e in self.persisted:
            self.add(e)
        self.flush()
        self.persisted = []


def key_sorted(roots):
    """A frame's roots as the kvdb iterator returns them."""
    return sorted(roots, key=lambda r: (r.validator, r.id))


def copy_store(store, key_order=False, rewind=0):
    """A fresh ``ao.Store`` holding what ``store`` holds."""
    s = ao.Store()
    s.epoch_state = store.epoch_state
    s.last_decided_frame = max(store.last_decided_frame - rewind, 0)
    for f, roots in store.roots.items():
        s.roots[f] = key_sorted(roots) if key_order else list(roots)
    s.confirmed = {eid: f for eid, f in store.confirmed.items() if f and f <= s.last_decided_frame}
    return s


def store_view(store):
    """What the tests compare of a store (ao.Store or the GPU wrapper's)."""
    roots = {}
    f = 1
    while True:
        rs = [getattr(r, "id", r) for r in store.get_frame_roots(f)]
        if not rs:
            break
        roots[f] = rs
        f += 1
    return dict(epoch=store.get_epoch(), last_decided_frame=store.last_decided_frame, roots=roots)


def store_from_state(state, validators, events):
    """``ao.Store`` of a GPU instance's ``state()``; ``events``: id -> event."""
    s = ao.Store()
    s.epoch_state = (int(state["epoch"]), validators)
    s.last_decided_frame = int(state["last_decided_frame"])
    ids, off, rev = state["ids"], state["root_off"], state["root_ev"]
    for f in range(1, len(off)):
        s.roots[f] = [ao.RootAndSlot(ids[k], f, events[ids[k]].creator) for k in rev[int(off[f - 1]):int(off[f])]]
    s.confirmed = {ids[k]: int(f) for k, f in enumerate(state["ev_confirmed_on"]) if f}
    return s


def state_from_store(store, ids, events):
    """The ``state()`` dict a GPU instance is restored from: ``store`` over the
    events ``ids`` (dense order), frames from the events."""
    pos = {eid: k for k, eid in enumerate(ids)}
    n_frames = max(store.roots) if store.roots else 0
    off, rev = [0], []
    for f in range(1, n_frames + 1):
        rev.extend(pos[r.id] for r in store.roots.get(f, []))
        off.append(len(rev))
    return dict(epoch=store.get_epoch(), last_decided_frame=store.last_decided_frame, ids=list(ids),
                ev_frame=np.array([events[i].frame for i in ids], dtype=np.uint32),
                ev_confirmed_on=np.array([store.confirmed.get(i, 0) for i in ids], dtype=np.uint32),
                root_off=np.array(off, dtype=np.uint64), root_ev=np.array(rev, dtype=np.uint32))


def _carry(t, prev):
    """The application's records survive the restart."""
    t.events = dict(prev.events)
    t.blocks = dict(prev.blocks)
    t.block_list = list(prev.block_list)
    t.epoch_blocks = dict(prev.epoch_blocks)
    t.last_block = prev.last_block
    t.apply_block = None
    return t


def restart_oracle(prev, processed, store):
    """A restarted oracle instance over ``store`` (a copy: it is written to)
    and a fresh index replaying ``processed``."""
    t = _carry(FakeLachesis.__new__(FakeLachesis), prev)
    t.store = store
    t.index = ReplayIndex(processed)
    t.lch = ao.IndexedLachesis(t.store, t.events.get, t.index)
    t.lch.bootstrap(t._begin_block)
    return t


def restart_gpu(prev, index_db, key_order=False, rewind=0, options=None):
    """Closes the GPU instance ``prev`` and rebuilds it through ``state()`` ->
    ``restore()``.  Returns (instance, the copied store it was restored from,
    the state dict handed to restore)."""
    from lachesis_hip import abft
    state = prev.lch.state()
    validators = prev.lch.validators
    store = copy_store(store_from_state(state, validators, prev.events), key_order, rewind)
    new_state = state_from_store(store, state["ids"], prev.events)
    prev.lch.close()
    t = _carry(FakeLachesis.__new__(FakeLachesis), prev)
    t.lch = abft.IndexedLachesis(validators, epoch=ao.FIRST_EPOCH)
    for k, v in (options or {}).items():
        t.lch.set_option(k, v)
    t.store = t.lch.store
    t.lch.restore(new_state, index_db, t.events.get, t._begin_block)
    return t, store, new_state


class IndexDB:
    """The index's kvdb tables ("S", "s", "b", "B") as a GPU index writes them
    back at its flushes (tests/test_gpu_restart.py checks them against the
    oracle's): a second index handle follows the abft instance's events."""

    def __init__(self, validators):
        import lachesis_hip
        self.ix = lachesis_hip.VecfcIndex()
        self.ix.reset(validators)
        self.db = {}

    def add(self, events):
        if events:
            self.ix.add_events(list(events))
            self.ix.flush(self.db)

    def copy(self):
        return {t: dict(v) for t, v in self.db.items()}

    def close(self):
        self.ix.ix.close()


# ---------------------------------------------------------------------------- CPU reference

def undecided_frames(store):
    """Frames above the last decided one that hold roots."""
    return [f for f in store.roots if f > store.last_decided_frame and store.roots[f]]


def cut_properties(store):
    """What makes a restart at this point exercise the rebuild:
    (root frames above the last decided one, some such frame holds two slots
    of one creator, some such frame's append order differs from key order)."""
    fs = undecided_frames(store)
    dup = any(len({r.validator for r in store.roots[f]}) < len(store.roots[f]) for f in fs)
    reorder = any(key_sorted(store.roots[f]) != list(store.roots[f]) for f in fs)
    return len(fs), dup, reorder


@functools.lru_cache(maxsize=None)
def oracle_reference(shape_key, every=10):
    """The uninterrupted oracle run of a shape (Build then Process per event)
    with a copy of its store after every ``every``-th event -- and three
    events later: creators take turns, so with 5 or 10 nodes every 10th event
    ends a turn of all nodes, where a forking creator's two roots of one frame
    were never seen undecided.  ``shape_key`` = (tuple(weights), cheaters,
    events per node, seed[, parent count])."""
    weights, cheaters, epn, seed = shape_key[:4]
    nodes, evs = gen_events(list(weights), cheaters, epn, seed, *shape_key[4:])
    o = FakeLachesis(dict(zip(nodes, weights)))
    cuts = {}
    for k, e in enumerate(evs):
        o.build(e)
        assert o.process(e) is None
        if (k + 1) % every in (0, 3 % every) and k + 1 < len(evs):
            cuts[k + 1] = (copy_store(o.store), len(o.block_list))
    return dict(nodes=nodes, evs=evs, frames={e.id: e.frame for e in evs}, blocks=list(o.block_list),
                last_block=o.last_block, store=store_view(o.store), confirmed=dict(o.store.confirmed),
                cuts=cuts, fake=o)


def clone_events(evs):
    """Fresh event objects (frame 0): an instance under test sets their frames."""
    return [tdag.Event(e.id, e.creator, e.seq, e.lamport, e.parents, e.name) for e in evs]


def fake_at(ref, cut):
    """The application's records of the reference run after ``cut`` events."""
    prev = FakeLachesis.__new__(FakeLachesis)
    n_blocks = ref["cuts"][cut][1]
    prev.events = {e.id: e for e in ref["evs"][:cut]}
    prev.block_list = list(ref["blocks"][:n_blocks])
    prev.blocks = {(b[0], b[1]): ref["fake"].blocks[(b[0], b[1])] for b in prev.block_list}
    prev.epoch_blocks = {1: n_blocks} if n_blocks else {}
    prev.last_block = (prev.block_list[-1][0], prev.block_list[-1][1]) if n_blocks else (0, 0)
    return prev


def pick_cuts(ref, n=8, need_dup=False):
    """At most ``n`` cut points of the reference run, evenly spread, among
    them one with two or more root frames above the last decided one, one
    whose append order differs from key order and (``need_dup``) one with two
    slots of one creator in such a frame."""
    all_cuts = sorted(ref["cuts"])
    step = max(len(all_cuts) // n, 1)
    cuts = all_cuts[step - 1::step][:n]
    props = {c: cut_properties(ref["cuts"][c][0]) for c in all_cuts}
    wants = [lambda p: p[0] >= 2]
    if len(ref["nodes"]) > 1:          # one validator: one slot per frame, one order
        wants.append(lambda p: p[2])
    if need_dup:
        wants.append(lambda p: p[1])
    for want in wants:
        if not any(want(props[c]) for c in cuts):
            cuts.append(next(c for c in all_cuts if want(props[c])))   # StopIteration: the shape never gets there
    while len(cuts) > n:               # drop one the conditions do not need
        spare = next(c for c in cuts if all(any(w(props[x]) for x in cuts if x != c) for w in wants))
        cuts.remove(spare)
    return sorted(cuts)
