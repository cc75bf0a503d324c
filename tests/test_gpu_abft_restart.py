"""Resuming an epoch on the GPU abft engine after a restart: lx_abft_restore
(include/lachesis_abft.h) over the state lx_abft_state_fetch hands out and the
index tables of a restart (tests/test_gpu_restart.py), against the abft
restatement restarted over the same copied store
(tests/test_abft_restart_oracle.py pins that flow, abft/restart_test.go).

Bit-exact after every restore -- last decided frame, root slots of every frame
in slot order, every event's frame and confirmed-on frame -- and at the end of
the epoch: frames, every block (Atropos, cheaters, confirmed events in
ApplyEvent order) and the last block, equal to a GPU instance and an oracle
that never stopped.
"""

import numpy as np
import pytest

from oracle import abft_oracle as ao
from abft_harness import FakeLachesis
from abft_restart_harness import (RESTART_SHAPES, IndexDB, clone_events, copy_store, cut_properties, fake_at,
                                  oracle_reference, pick_cuts, restart_gpu, restart_oracle, store_from_state,
                                  store_view)

pytestmark = pytest.mark.gpu

LX_ERR_ARG, LX_ERR_STATE = -1, -4

# tile edges of the rebuild (64 x 64 event x root tiles, 32-column chunks):
# tests/test_gpu_abft.py::SHAPES[7] -- 40 validators, 4 cheaters: more than 32
# branch columns, the fork path, two slots of one creator in a frame -- and 70
# fork-free validators: 70 slots per frame, a partial second tile both ways
TILE_SHAPES = [
    ([5 + (i % 7) for i in range(40)], 4, 15, 8, 8),
    ([1 + (i % 3) for i in range(70)], 0, 10, 10, 9),
]


def shape_key(shape):
    return (tuple(shape[0]),) + tuple(shape[1:])


_gpu_runs = {}


def uninterrupted_gpu(key, fc16):
    """One GPU instance that never stops (Build then Process per event)."""
    if (key, fc16) not in _gpu_runs:
        ref = oracle_reference(key)
        evs = clone_events(ref["evs"])
        t = FakeLachesis(dict(zip(ref["nodes"], key[0])), backend="gpu", options={"fc16": fc16})
        for e in evs:
            t.build(e)
            assert t.process(e) is None
        _gpu_runs[(key, fc16)] = dict(frames={e.id: e.frame for e in evs}, blocks=list(t.block_list),
                                      last_block=t.last_block, store=store_view(t.store))
        t.lch.close()
    return _gpu_runs[(key, fc16)]


def advance(t, db, evs, mode, claim):
    """Processes evs on the instance and on the index that writes the tables."""
    kind = mode[0]
    if kind == "event":
        for e in evs:
            t.build(e)
            assert t.process(e) is None
    else:
        for e in evs:
            e.frame = claim[e.id]
        for lo in range(0, len(evs), 23):
            part = evs[lo:lo + 23]
            consumed, err = t.process_batch(part, claimed=True)
            assert err is None and consumed == len(part)
    db.add(evs)


def check_restored(t, ref, cut, store_copy, events):
    """Everything the store answers after the restore equals the oracle
    restored from the same copied store.  Returns the oracle's view."""
    o = restart_oracle(fake_at(ref, cut), ref["evs"][:cut], copy_store(store_copy))
    want = store_view(o.store)
    got = store_view(t.store)
    assert got == want, cut
    for e in events[:cut]:
        assert t.lch.frame_of(e.id) == ref["frames"][e.id], (cut, e)
        assert t.store.get_event_confirmed_on(e.id) == o.store.confirmed.get(e.id, 0), (cut, e)
    assert len(t.block_list) == len(o.block_list) == ref["cuts"][cut][1], cut   # no callback during the restore
    return want


def run_restarts(key, fc16, key_order, mode, cuts=None, rewind_at=None):
    """A GPU instance closed and rebuilt at the cut points; returns its final
    results and the stats / store copies seen at the restores."""
    ref = oracle_reference(key)
    need_dup = key[1] > 0
    cuts = pick_cuts(ref, need_dup=need_dup) if cuts is None else cuts
    props = [cut_properties(ref["cuts"][c][0]) for c in cuts]
    assert any(p[0] >= 2 for p in props)
    assert not need_dup or any(p[1] for p in props)
    assert len(key[0]) == 1 or any(p[2] for p in props)
    options = {"fc16": fc16}
    if mode[0] == "batch":
        options.update(claimed_batch=mode[1], elect_ahead=mode[2])
    evs = clone_events(ref["evs"])
    t = FakeLachesis(dict(zip(ref["nodes"], key[0])), backend="gpu", options=options)
    db = IndexDB(t.lch.validators)
    seen = []
    done = 0
    try:
        for cut in cuts:
            advance(t, db, evs[done:cut], mode, ref["frames"])
            done = cut
            # the state handed out is the oracle's store at this point (slot
            # order too, unless an earlier restart sorted the slots it loaded)
            if rewind_at is None:
                before = store_from_state(t.lch.state(), t.lch.validators, t.events)
                got, want = store_view(before), store_view(ref["cuts"][cut][0])
                if key_order:
                    got["roots"] = {f: sorted(r) for f, r in got["roots"].items()}
                    want["roots"] = {f: sorted(r) for f, r in want["roots"].items()}
                assert got == want, cut
                assert before.confirmed == ref["cuts"][cut][0].confirmed, cut
            rewind = 2 if rewind_at == cut else 0
            t, store_copy, state = restart_gpu(t, db.copy(), key_order, rewind, options)
            stats = t.lch.last_stats()
            view = check_restored(t, ref, cut, store_copy, evs)
            seen.append(dict(cut=cut, stats=stats, store=store_copy, state=state, view=view,
                             state_after=t.lch.state()))
        advance(t, db, evs[done:], mode, ref["frames"])
        return dict(frames={e.id: t.lch.frame_of(e.id) for e in evs}, ev_frames={e.id: e.frame for e in evs},
                    blocks=list(t.block_list), last_block=t.last_block, store=store_view(t.store),
                    confirmed={e.id: t.store.get_event_confirmed_on(e.id) for e in evs}, seen=seen)
    finally:
        t.lch.close()
        db.close()


MODES = [("event",), ("batch", 1, 3), ("batch", 0, 0)]
PARITY = [(s, 1) for s in RESTART_SHAPES] + [(s, 0) for s in RESTART_SHAPES if s[1] == 0]


@pytest.mark.parametrize("mode", MODES, ids=["event", "batch_cb1_ea3", "batch_cb0_ea0"])
@pytest.mark.parametrize("key_order", [False, True])
@pytest.mark.parametrize("shape,fc16", PARITY, ids=["%d-fc16_%d" % (RESTART_SHAPES.index(s), f) for s, f in PARITY])
def test_restart_parity(shape, fc16, key_order, mode):
    """Restarts at up to 8 cut points; the run continues event by event (Build
    then Process) or in batches with claimed frames, and ends like the
    instances that never stopped."""
    key = shape_key(shape)
    ref = oracle_reference(key)
    assert len(ref["blocks"]) >= 3
    got = run_restarts(key, fc16, key_order, mode)
    gpu = uninterrupted_gpu(key, fc16)
    assert got["frames"] == got["ev_frames"] == ref["frames"] == gpu["frames"]
    assert got["blocks"] == ref["blocks"] == gpu["blocks"]
    assert got["last_block"] == ref["last_block"] == gpu["last_block"]
    assert got["confirmed"] == {e.id: ref["confirmed"].get(e.id, 0) for e in ref["evs"]}
    if not key_order:
        assert got["store"] == ref["store"] == gpu["store"]
    else:
        assert got["store"]["last_decided_frame"] == ref["store"]["last_decided_frame"]
        assert {f: sorted(r) for f, r in got["store"]["roots"].items()} == \
               {f: sorted(r) for f, r in ref["store"]["roots"].items()}
    # state() of a restored instance is the state it was restored from
    for s in got["seen"]:
        for k in ("epoch", "last_decided_frame", "ids"):
            assert s["state_after"][k] == s["state"][k], (s["cut"], k)
        for k in ("ev_frame", "ev_confirmed_on", "root_off", "root_ev"):
            assert np.array_equal(s["state_after"][k], s["state"][k]), (s["cut"], k)


def rebuilt_pairs(store):
    """(frames, pairs) of the rebuild: every slot of a frame above the last
    decided one against every slot of the frame below it."""
    fs = [f for f in store.roots if f > store.last_decided_frame and f >= 2]
    return len(fs), sum(len(store.roots[f]) * len(store.roots[f - 1]) for f in fs)


@pytest.mark.parametrize("key_order", [False, True])
@pytest.mark.parametrize("shape", TILE_SHAPES, ids=["v40_forks", "v70"])
def test_restart_tile_edges_and_launch_count(shape, key_order):
    """The rebuild over more than 32 branch columns with duplicate-creator
    slots, and over frames of 70 slots (a partial second tile in both
    directions); every restore rebuilds all its frames in one root-FC launch."""
    key = shape_key(shape)
    ref = oracle_reference(key)
    assert len(ref["blocks"]) >= 3
    got = run_restarts(key, 1, key_order, ("batch", 1, 2))
    assert got["frames"] == ref["frames"]
    assert got["blocks"] == ref["blocks"]
    assert got["last_block"] == ref["last_block"]
    if shape[1] == 0:
        assert max(len(r) for r in ref["store"]["roots"].values()) > 64
    n_frames = set()
    for s in got["seen"]:
        frames, pairs = rebuilt_pairs(s["store"])
        n_frames.add(frames)
        # one merged launch of the one root-FC kernel variant the epoch takes
        assert s["stats"]["fc_launches"] == (1 if frames else 0), s["cut"]
        assert s["stats"]["fc_pairs"] == pairs, s["cut"]
        assert s["stats"]["frame_steps"] == frames, s["cut"]
    assert max(n_frames) >= 2 and len(n_frames) >= 2   # the count does not follow the frames


@pytest.mark.parametrize("key_order", [False, True])
@pytest.mark.parametrize("shape", [RESTART_SHAPES[1], RESTART_SHAPES[4], RESTART_SHAPES[6]], ids=["1", "4", "6"])
def test_restart_rewound(shape, key_order):
    """The last decided frame rewound by two: the restore decides the two
    frames again without a callback, and the events only they confirmed keep
    confirmed-on 0 (check_restored, against the oracle restored from the same
    copy); the run then ends like the oracle continued from that copy."""
    key = shape_key(shape)
    ref = oracle_reference(key)
    cuts = pick_cuts(ref, need_dup=key[1] > 0)
    cut = next(c for c in cuts[len(cuts) // 2:] if ref["cuts"][c][0].last_decided_frame >= 3)
    got = run_restarts(key, 1, key_order, ("batch", 1, 3), cuts=cuts, rewind_at=cut)
    s = next(x for x in got["seen"] if x["cut"] == cut)
    store = ref["cuts"][cut][0]
    assert s["store"].last_decided_frame == store.last_decided_frame - 2
    assert s["view"]["last_decided_frame"] == store.last_decided_frame
    assert s["stats"]["vote_launches"] > 0
    redecided = [eid for eid, f in store.confirmed.items() if f > s["store"].last_decided_frame]
    assert redecided
    assert all(int(s["state_after"]["ev_confirmed_on"][s["state"]["ids"].index(eid)]) == 0 for eid in redecided)
    # the oracle over the same copies: same cuts, same key order, same rewind
    o = None
    for c in cuts:
        if c < cut:
            continue
        if c == cut:
            o = restart_oracle(fake_at(ref, c), ref["evs"][:c], copy_store(s["store"]))
        else:
            o = restart_oracle(o, ref["evs"][:c], copy_store(o.store, key_order))
        nxt = next((x for x in cuts if x > c), len(ref["evs"]))
        for e in ref["evs"][c:nxt]:
            assert o.process(e) is None
    assert got["blocks"] == o.block_list
    assert got["confirmed"] == {e.id: o.store.confirmed.get(e.id, 0) for e in ref["evs"]}
    assert got["frames"] == ref["frames"]
    assert [b[:4] for b in got["blocks"]] == [b[:4] for b in ref["blocks"]]


# ---------------------------------------------------------------------------- refusals

def _arrays(lch, state, events):
    evs = [events[i] for i in state["ids"]]
    lch.pos, lch.evs = {}, []
    return lch._dense(evs)


def test_restore_refusals():
    """Every inconsistency of the input is refused with a message before
    anything is built; the handle stays usable: bootstrap works afterwards, and
    a restore on a bootstrapped handle is LX_ERR_STATE."""
    from lachesis_hip import LxError, abft
    from lachesis_hip.vecfc import load_epoch_tables
    key = shape_key(RESTART_SHAPES[2])
    ref = oracle_reference(key)
    cut = next(c for c in sorted(ref["cuts"]) if ref["cuts"][c][0].last_decided_frame >= 2)
    evs = clone_events(ref["evs"])
    for e in evs:
        e.frame = ref["frames"][e.id]
    events = {e.id: e for e in evs}
    t = FakeLachesis(dict(zip(ref["nodes"], key[0])), backend="gpu")
    db = IndexDB(t.lch.validators)
    consumed, err = t.process_batch(evs[:cut])
    assert err is None and consumed == cut
    db.add(evs[:cut])
    validators = t.lch.validators
    good = t.lch.state()
    t.lch.close()
    tables = db.copy()
    db.close()
    n, ldf = len(good["ids"]), int(good["last_decided_frame"])
    n_frames = len(good["root_off"]) - 1
    sp_root = next(k for k in range(n) if ao.self_parent(events[good["ids"][k]]) is not None
                   and good["ev_frame"][k] == n_frames)

    def mutated(**kw):
        s = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in good.items()}
        for k, v in kw.items():
            s[k] = v(s[k]) if callable(v) else v
        return s

    def bump(i, d):
        def f(a):
            a[i] += d
            return a
        return f

    def swap_root_off(a):
        a[1], a[2] = a[2], a[1]
        return a

    def foreign_slot(a):
        # a root of the last frame listed in frame 1 as well
        a[0] = sp_root
        return a

    bad = {
        "root index >= n_events": mutated(root_ev=bump(0, n)),
        "slot outside (frame(self-parent), frame]": mutated(root_ev=foreign_slot),
        "last decided frame above the roots table": mutated(last_decided_frame=n_frames + 1),
        "confirmed above the last decided frame": mutated(ev_confirmed_on=bump(0, ldf + 1 - int(good["ev_confirmed_on"][0]))),
        "non-monotone root_off": mutated(root_off=swap_root_off),
    }
    lch = abft.IndexedLachesis(validators, epoch=ao.FIRST_EPOCH)
    w = validators.weights

    def reload():
        lch.ix.reset(w)
        load_epoch_tables(lch.ix, validators, tables, events.get, order=good["ids"])

    for name, state in bad.items():
        reload()
        rc = abft.restore_arrays(lch.L, lch.h, state, w, *_arrays(lch, good, events), None)
        assert rc == LX_ERR_ARG, name
        assert lch.L.lx_abft_last_error(lch.h), name
    # n_events != lx_num_events(index)
    reload()
    short = {k: (v[:-1] if k in ("ev_frame", "ev_confirmed_on") else v) for k, v in good.items()}
    creator, seq, off, flat = _arrays(lch, good, events)
    rc = abft.restore_arrays(lch.L, lch.h, short, w, creator[:-1], seq[:-1], off[:-1], flat, None)
    assert rc in (LX_ERR_ARG, LX_ERR_STATE) and b"events" in lch.L.lx_abft_last_error(lch.h)
    # an index in the middle of loading
    lch.ix.reset(w)
    half = good["ids"][:cut // 2]
    e0 = [events[i] for i in half]
    pos = {eid: k for k, eid in enumerate(half)}
    lch.ix.load_rows([validators.idxs[e.creator] for e in e0], [e.seq for e in e0],
                     np.cumsum([0] + [len(e.parents) for e in e0]), [pos[p] for e in e0 for p in e.parents],
                     b"".join(tables["b"][i] for i in half), [tables["S"][i] for i in half],
                     [tables["s"][i] for i in half])
    rc = abft.restore_arrays(lch.L, lch.h, good, w, *_arrays(lch, good, events), None)
    assert rc == LX_ERR_STATE and lch.L.lx_abft_last_error(lch.h)
    # a failed restore leaves the handle not bootstrapped: the good state still restores ...
    lch.restore(good, tables, events.get)
    assert lch.store.last_decided_frame == ldf
    with pytest.raises(LxError) as ex:
        lch.restore(good, tables, events.get)
    assert ex.value.code == LX_ERR_STATE and "already bootstrapped" in str(ex.value)
    lch.close()
    # ... and so does a plain bootstrap, after which a restore is refused
    lch = abft.IndexedLachesis(validators, epoch=ao.FIRST_EPOCH)
    reload()
    assert abft.restore_arrays(lch.L, lch.h, bad["non-monotone root_off"], w, *_arrays(lch, good, events), None) == LX_ERR_ARG
    lch.bootstrap(None)
    consumed, err = lch.process_batch(evs[:cut])
    assert err is None and consumed == cut and lch.store.last_decided_frame == ldf
    with pytest.raises(LxError) as ex:
        lch.restore(good, tables, events.get)
    assert ex.value.code == LX_ERR_STATE
    lch.close()


def test_restore_refuses_sharded_index():
    import ctypes
    from lachesis_hip import Index, abft
    from lachesis_hip.capi import vp
    ix = Index(shard_rank=0, shard_count=2)
    h = vp()
    assert ix.L.lx_abft_create(ix.h, ctypes.byref(h)) == 0
    ix.reset([1, 1, 1, 1])
    empty = dict(epoch=1, last_decided_frame=0, ev_frame=[], ev_confirmed_on=[], root_off=[0], root_ev=[])
    rc = abft.restore_arrays(ix.L, h, empty, [1, 1, 1, 1], [], [], [0], [], None)
    assert rc == LX_ERR_STATE and ix.L.lx_abft_last_error(h)
    ix.L.lx_abft_destroy(h)
    ix.close()


# ---------------------------------------------------------------------------- dense path

def test_dense_restore_mid_epoch_c4():
    """DenseLachesis restored in the middle of the committed abft_c4 epoch
    (100 validators, 10 % double-signers, 100k events) ends on the fixture's
    frames and blocks."""
    from lachesis_hip import Index, abft, tools
    from test_gpu_abft import blocks_of, load_golden
    g = load_golden("c4")
    V, epn, P, ch, fk, seed = map(int, g["config"])
    d = tools.gen_dag(V, epn, P, cheaters=ch, forks=fk, seed=seed)
    N, cut = len(d), len(d) // 2
    first = abft.DenseLachesis(g["weights"], event_capacity=N)
    c, s, off, par = d.slice(0, cut)
    rc, consumed, out = first.process_batch(c, s, off, par, g["frames"][:cut])
    assert rc == 0 and consumed == cut
    state = first.state()
    blocks = list(first.blocks)
    first.close()
    assert 0 < state["last_decided_frame"] < len(state["root_off"]) - 1
    # the index tables of the first half, as its flush writes them back
    ix = Index(event_capacity=N)
    ix.reset(g["weights"])
    ix.add_batch(c, s, off, par)
    tables = ix.writeback()
    ix.close()
    lch = abft.DenseLachesis(g["weights"], event_capacity=N, bootstrap=False)
    lch.restore(state, c, s, off, par, tables)
    st = lch.last_stats()
    assert st["fc_launches"] == 1 and st["fc_pairs"] > 0
    assert lch.last_decided_frame() == state["last_decided_frame"]
    again = lch.state()
    assert all(np.array_equal(again[k], state[k]) for k in state)
    c2, s2, off2, par2 = d.slice(cut, N)
    rc, consumed, out2 = lch.process_batch(c2, s2, off2, par2, g["frames"][cut:])
    assert rc == 0 and consumed == N - cut
    assert np.array_equal(np.concatenate([out, out2]), g["frames"])
    assert [len(lch.frame_roots(f)) for f in range(len(g["roots_per_frame"]))] == list(g["roots_per_frame"])
    assert blocks + lch.blocks == blocks_of(g)
    assert np.array_equal(lch.state()["ev_confirmed_on"] > 0, np.isin(np.arange(N), g["confirmed"]))
    lch.close()
