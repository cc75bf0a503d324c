"""The rule lx_abft_build_progress rests on (tests/progress_model.py), on the
CPU.  The yardstick: add the candidate to the C oracle, read its real
HighestBefore row and the roots' real LowestAfter rows, count as forklessCause
counts (no virtual row, no correction), drop it again -- the model's pair
stakes for the candidate that is NOT added must equal those sums at every
frame of its climb."""

import numpy as np
import pytest

import build_model as bm
import progress_model as pm

WEIGHTED = ((3, 12, 3, 0, 0, 2), (5, 2, 2))


def checkpoints(n):
    return sorted({max(1, n // 5), max(1, n // 2), n})


def walk(shape, weights=None):
    """Every tip candidate of the shape at the three checkpoints: yields
    (model, candidate, row, spf, Build frame)."""
    ep = bm.Epoch.of_shape(shape, weights=list(weights) if weights else None)
    V, P = shape[0], shape[2]
    for upto in checkpoints(len(ep.events)):
        ep.advance(upto)
        m = pm.ProgressModel(ep)
        for c in ep.tip_candidates(sorted({0, 1, max(P - 1, 0), V - 1})):
            spf, F = m.frame(c)
            assert F == ep.oracle_frame(c)
            assert (spf, F) == m.build_frame(c)
            yield m, c, m.virtual_row(c), spf, F


@pytest.mark.parametrize("shape", bm.SHAPES)
def test_pair_stakes_equal_the_sums_on_real_rows(shape):
    steps = 0
    for m, c, row, spf, F in walk(shape):
        o = m.ep.orc
        assert o.add(c.creator, c.seq, c.parents) == 0
        try:
            e = o.num_events() - 1
            for f in range(max(spf, 1), F + 1):
                rs = m.roots.get(f, [])
                exp = pm.oracle_pair_stakes(o, e, rs, m.w, m.branch_creator, m.V)
                got = m.pair_stakes(c, row, rs)
                assert np.array_equal(got, exp), (c.tip, c.k, f)
                # ForklessCause itself, and the frame loop's condition
                assert [bool(x >= m.quorum) for x in got] == [bool(o.forkless_cause(e, r)) for r in rs]
                p = m.progress(c, f, row)
                assert (p["stake"] >= m.quorum) == (f < F) or F == spf + bm.BUILD_CAP
                assert p["root_stake"] == int(np.minimum(exp, m.quorum).sum())
                steps += 1
        finally:
            o.drop_not_flushed()
    assert steps >= (0 if shape[0] == 1 else 30)


@pytest.mark.parametrize("shape,weights", [(s, None) for s in bm.SHAPES if s[0] > 1] + [WEIGHTED],
                         ids=lambda x: "-".join(map(str, x)) if x else "eq")
def test_inputs_carry_signal(shape, weights):
    """At the Build frame: candidates strictly between nothing and a quorum,
    pairs strictly between, and pairs that are caused."""
    part_cands = part_pairs = caused = 0
    for m, c, row, spf, F in walk(shape, weights):
        p = m.progress(c, F, row)
        assert p["stake"] < m.quorum
        part_cands += 0 < p["stake"] < m.quorum
        part_pairs += sum(0 < s < m.quorum for _, s in p["pairs"])
        caused += sum(s >= m.quorum for _, s in p["pairs"])
        assert p["n_caused"] == sum(s >= m.quorum for _, s in p["pairs"])
    assert part_cands >= 10 and part_pairs >= 10 and caused >= 10, (part_cands, part_pairs, caused)


def test_single_validator_answers_zeros():
    """V = 1: every event is a root of a new frame, the Build frame has no
    roots yet."""
    n = 0
    for m, c, row, spf, F in walk((1, 6, 1, 0, 0, 1)):
        assert F == spf + 1 and F not in m.roots
        p = m.progress(c, F, row)
        assert (p["n_roots"], p["n_caused"], p["stake"], p["root_stake"], p["pairs"]) == (0, 0, 0, 0, [])
        n += 1
    assert n >= 3


def test_indexed_events_against_their_frames():
    """An indexed event's stake is below the quorum at its own frame and at or
    above it at each earlier frame back to its self-parent's frame; a root
    leaves its own slot out of the sums and keeps it in the pair list."""
    ep = bm.Epoch.of_shape((12, 30, 4, 3, 5, 2))
    ep.advance(len(ep.events))
    m = pm.ProgressModel(ep)
    own_slots = 0
    for e in range(m.n):
        f = int(m.frames[e])
        ev = ep.events[e]
        spf = int(m.frames[ep.pos(ev.parents[0])]) if ev.seq > 1 else 0
        p = m.event_progress(e, f)
        assert p["stake"] < m.quorum, e
        for g in range(max(spf, 1), f):
            assert m.event_progress(e, g)["stake"] >= m.quorum, (e, g)
        for r, s in p["pairs"]:
            assert (s >= m.quorum) == bool(ep.orc.forkless_cause(e, r))
        if e in m.roots.get(f, []):
            own_slots += 1
            assert p["n_roots"] == len(p["pairs"])
            assert p["n_caused"] == sum(s >= m.quorum for r, s in p["pairs"] if r != e)
    assert own_slots > 10
