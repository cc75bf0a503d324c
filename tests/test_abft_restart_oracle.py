"""The flow of abft/restart_test.go on the abft restatement alone: an instance
is restarted over a copy of its store (Bootstrap over a non-empty Store,
oracle/abft_oracle.py bootstrap_orderer -> _bootstrap_election ->
_process_known_roots; abft/bootstrap.go:34-55, event_processing.go:102-146)
and must go on exactly like an instance that never stopped.

This pins the semantics the GPU restart tests (tests/test_gpu_abft_restart.py)
are judged against, and asserts that the shapes put the restart where the
GPU's rebuild has work to do.

Rewound copies (the last decided frame lowered by two, the confirmed entries
above it dropped): Bootstrap decides the two frames again before the
callbacks are assigned (abft/lachesis.go:92-98), so no block is applied for
them and the events only they confirmed stay unconfirmed until a later block's
walk reaches them.  Frames, roots, decided frames, Atropoi and cheaters are
those of the uninterrupted run; the confirmed-on frame of those events and the
ApplyEvent lists of later blocks are not, and are checked for exactly that
difference.
"""

import pytest

from abft_restart_harness import (RESTART_SHAPES, copy_store, cut_properties, fake_at, oracle_reference,
                                  restart_oracle, store_view)


def shape_key(shape):
    return (tuple(shape[0]),) + tuple(shape[1:])


def continue_from(ref, cut, store):
    """Restart at ``cut`` over ``store`` and process the rest of the epoch."""
    evs = ref["evs"]
    t = restart_oracle(fake_at(ref, cut), evs[:cut], store)
    after = dict(store_view(t.store), confirmed=dict(t.store.confirmed), n_blocks=len(t.block_list))
    for e in evs[cut:]:
        assert t.process(e) is None
    return t, after


@pytest.mark.parametrize("rewind", [0, 2])
@pytest.mark.parametrize("key_order", [False, True])
@pytest.mark.parametrize("shape", RESTART_SHAPES, ids=[str(i) for i in range(len(RESTART_SHAPES))])
def test_restart_at_every_tenth_event(shape, key_order, rewind):
    """One restart per cut point (every 10th event and three events later,
    abft_restart_harness.oracle_reference), then the rest of the epoch."""
    ref = oracle_reference(shape_key(shape))
    assert len(ref["blocks"]) >= 3
    for cut, (store, n_blocks) in ref["cuts"].items():
        copy = copy_store(store, key_order, rewind)
        ldf0 = copy.last_decided_frame
        t, after = continue_from(ref, cut, copy)
        # Bootstrap: no block callback; a rewound copy decides its frames again
        assert after["n_blocks"] == n_blocks, cut
        assert after["last_decided_frame"] == store.last_decided_frame, cut
        got = store_view(t.store)
        want = ref["store"]
        assert got["last_decided_frame"] == want["last_decided_frame"] and got["epoch"] == want["epoch"], cut
        assert {f: sorted(r) for f, r in got["roots"].items()} == {f: sorted(r) for f, r in want["roots"].items()}, cut
        if not key_order:
            assert got["roots"] == want["roots"], cut
        assert t.last_block == ref["last_block"], cut
        assert [b[:4] for b in t.block_list] == [b[:4] for b in ref["blocks"]], cut
        redecided = {eid for eid, f in store.confirmed.items() if f > ldf0}
        if not redecided:
            assert t.block_list == ref["blocks"], cut
            assert t.store.confirmed == ref["confirmed"], cut
            continue
        # rewound: the events of the frames decided again are confirmed by a
        # later block instead (or not at all, if the epoch ends first)
        assert after["confirmed"] == {eid: f for eid, f in store.confirmed.items() if f <= ldf0}, cut
        for eid, f in ref["confirmed"].items():
            g = t.store.confirmed.get(eid, 0)
            assert (g == 0 or g > store.last_decided_frame) if eid in redecided else g == f, (cut, eid)
        extra = sorted(set(x for b in t.block_list for x in b[4]) - set(x for b in ref["blocks"] for x in b[4]))
        assert extra == [], cut
        assert all(set(b[4]) <= set(r[4]) | redecided for b, r in zip(t.block_list, ref["blocks"])), cut


@pytest.mark.parametrize("shape", RESTART_SHAPES, ids=[str(i) for i in range(len(RESTART_SHAPES))])
def test_shapes_exercise_the_rebuild(shape):
    """Per shape: some cut has roots in two or more frames above the last
    decided one, some cut's slot order differs from key order (not with one
    validator: one slot per frame), and with cheaters some cut has a frame
    above the last decided one holding two slots of one creator."""
    ref = oracle_reference(shape_key(shape))
    props = [cut_properties(store) for store, _ in ref["cuts"].values()]
    assert any(p[0] >= 2 for p in props)
    if len(shape[0]) > 1:
        assert any(p[2] for p in props)
    if shape[1]:
        assert any(p[1] for p in props)
