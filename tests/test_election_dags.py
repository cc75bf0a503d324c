"""The scenarios of tests/election_dags.py reach the election branches they are
there for -- asserted from the C oracle alone, so that a change of the
generator cannot silently turn tests/test_gpu_election_dags.py into a test of
the ordinary path.  CPU only.

An Atropos whose creator idx is >= 64 cannot be found inside the first subject
window [0, 64): every subject of it was decided "no" and the window was
doubled; idx >= 128 takes two doublings.  An election's round count is (frame
of the event at which the oracle emits block F) - F, the oracle fed event by
event.
"""

from collections import Counter

import numpy as np
import pytest

import election_dags as ed
from abft_harness import FakeLachesis

_cache = {}


def oracle(name):
    if name not in _cache:
        w, d = ed.scenario(name)
        _cache[name] = (w, d, ed.oracle_run(w, d, by_event=True))
    return _cache[name]


def atropos_creators(d, res):
    return [int(d.creator[b[2]]) for b in res["blocks"]]


def rounds_of(res):
    return [res["rounds"][f] for f in sorted(res["rounds"])]


def test_generator_shape():
    """Add order, one event per active validator and level, P distinct
    creators per parent list with the self-parent first, tips of the level
    before."""
    w, d = ed.scenario("head_silent_return")
    assert len(d) == 200 * 40 - 66 * 20 == 6680
    assert np.array_equal(d.level_ends, np.cumsum([0] + [134 if 8 <= l < 28 else 200 for l in range(40)]))
    for e in range(len(d)):
        ps = d.par[int(d.poff[e]):int(d.poff[e + 1])]
        assert all(p < d.level_ends[d.level[e]] for p in ps)
        cs = [int(d.creator[p]) for p in ps]
        assert len(set(cs)) == len(cs) == (12 if d.level[e] else 0)
        if d.level[e]:
            assert cs[0] == d.creator[e] and d.seq[e] == d.seq[ps[0]] + 1
    silent = d.level_ends[8]
    assert d.creator[silent:d.level_ends[28]].min() == 66


def test_head_silent_return():
    w, d, res = oracle("head_silent_return")
    assert atropos_creators(d, res) == [0, 0, 66, 66, 0]   # before, during (widened) and after the outage
    assert res["last"] == 5 and int(res["frames"].max()) == 7
    held = Counter(e for roots in res["roots"] for e in roots)
    multi = [e for e, k in held.items() if k >= 2]
    # the head's first events after the outage: a root of every frame they pass
    assert len(multi) == 66 and all(d.creator[e] < 66 and d.level[e] == ed.OUTAGE[1] for e in multi)
    assert rounds_of(res) == [2] * 5


def test_head_never():
    w, d, res = oracle("head_never")
    assert atropos_creators(d, res) == [66, 66]            # 64 <= 66 < 128: one widening
    assert len(d) == 134 * 24 and res["last"] == 2


def test_head_never_two():
    w, d, res = oracle("head_never_two")
    assert atropos_creators(d, res) == [130, 130]          # 128 <= 130 < 256: two widenings
    assert len(d) == 270 * 20 and res["last"] == 2


@pytest.mark.parametrize("name,longest,n4", [("long_rounds", 9, 6), ("long_rounds5", 5, 2), ("long_rounds7", 4, 1),
                                             ("long_rounds_unequal", 7, 6)])
def test_long_rounds(name, longest, n4):
    w, d, res = oracle(name)
    r = rounds_of(res)
    assert max(r) == longest and sum(x >= 4 for x in r) == n4
    assert len(res["blocks"]) >= 13


def test_long_rounds_weighted_is_short():
    """Weights [4, 2, 1, 1]: validator 0 is in every quorum (6 of 8), every
    root of frame F + 1 forkless-causes its root of frame F, so subject 0 is
    decided yes in round 2 of every election of a real DAG (the four rounds of
    the golden "4rounds" case need its fake observe relation)."""
    w, d, res = oracle("long_rounds_weighted")
    assert set(rounds_of(res)) == {2} and len(res["blocks"]) >= 20
    assert set(atropos_creators(d, res)) == {0}


@pytest.mark.parametrize("name", ["long_rounds", "long_rounds_weighted", "long_rounds_unequal"])
def test_python_restatement_agrees(name):
    """oracle/abft_oracle.py through FakeLachesis, event by event: the C
    oracle's frames and blocks."""
    w, d, res = oracle(name)
    wmap, evs = ed.as_events(w, d)
    t = FakeLachesis(wmap)
    for e in evs:
        t.build(e)
        assert t.process(e) is None
    assert [e.frame for e in evs] == res["frames"].tolist()
    want = [(ep, f, a + 1, ch, tuple(x + 1 for x in conf)) for ep, f, a, ch, conf in res["blocks"]]
    assert t.block_list == want
    assert t.store.last_decided_frame == res["last"]


def first_decider(w, d, roots, F, upto):
    """The event at which oracle.abft_oracle.Election decides frame F when it
    is fed the roots of frames F + 1 .. upto in event order (None: not within
    them), over the C index's ForklessCause."""
    from oracle import abft_oracle as ao
    from oracle import corc, pos
    ix = corc.OracleIndex(w)
    ix.add_batch(d.creator, d.seq, d.poff, d.par)
    vals = pos.Validators({i + 1: x for i, x in enumerate(w)})
    slots = {f: [ao.RootAndSlot(e, f, int(d.creator[e]) + 1) for e in roots[f]] for f in range(F, upto + 1)}
    el = ao.Election(vals, F, lambda a, b: bool(ix.forkless_cause(a, b)), lambda f: slots.get(f, []))
    for r in sorted((r for f in range(F + 1, upto + 1) for r in slots[f]), key=lambda r: r.id):
        if el.process_root(r) is not None:
            return r.id
    return None


def test_lagger_return():
    """Election 3: the first root to decide it within two rounds (frames 4,
    5) is the lagging validator's first event after its pause, event 48 -- but
    event 45, a root of frame 6, decides it in round 3 and is older.  Deciding
    frame 3 from two rounds of votes alone would name event 48; the block is
    due at event 45, which shows where a seal on frame 3 ends the epoch."""
    w, d, res = oracle("lagger_return")
    nf = len(res["roots"]) - 1
    assert first_decider(w, d, res["roots"], 3, 5) == 48 and d.creator[48] == 3 and d.level[48] == 12
    assert first_decider(w, d, res["roots"], 3, nf) == 45 and res["frames"][45] == 6
    sealed = ed.oracle_run(w, d, seal=lambda epoch, frame: w if frame == 3 else None)
    assert sealed["consumed"] == 46 and sealed["epoch"] == 2 and [b[1] for b in sealed["blocks"]] == [1, 2, 3]
