"""What fork evidence rests on (tests/fork_evidence_model.py), on the CPU: the
naive definition (two events of one creator with one seq among a head's
ancestors) holds exactly where the C oracle's HighestBefore rows carry the fork
marker, raw and merged; the branch-interval rule the kernel computes, evaluated
on the oracle's rows, gives the model's canonical pair; the creators with
evidence at an Atropos are the block's cheaters; and the hand-built DAGs of
tests/fork_evidence_dags.py have the answers they were built for."""

import numpy as np
import pytest

import ancestry_model as am
import fork_evidence_dags as fd
import fork_evidence_model as fm
from oracle import vecfc_oracle as vo

FORK_SHAPES = [s for s in am.PAIR_SHAPES if s[3]]
# (head, creator) pairs with evidence, and whether a slot holds three or more events
QUOTED = {
    (12, 30, 4, 3, 5, 2): (993, True),
    (40, 12, 6, 8, 4, 3): (3059, True),
    (9, 20, 3, 9, 4, 7): (1364, True),
    (257, 3, 8, 5, 2, 6): (554, False),
    (20, 15, 4, 6, 6, 11): (1476, True),
    (6, 40, 3, 3, 10, 5): (673, True),
}


def _merged_marks(m):
    """[head, creator]: the merged HighestBefore entry is the fork marker."""
    o = m.rows()[0]
    V = len(m.validators.weights)
    out = np.zeros((m.n, V), dtype=bool)
    for i in range(m.n):
        r = np.frombuffer(o.merged_hb(i), dtype=np.uint32).reshape(-1, 2)
        out[i, :len(r)] = (r[:, 0] == 0) & (r[:, 1] == vo.MAX_INT32)
    return out


def _marks_equal_evidence(m):
    """evidence <=> the raw row marks the creator (its original branch, and
    with it every branch the row holds) <=> the merged flag."""
    _, branch, _, hb_mark, _ = m.rows()
    br = fm.Branches(m)
    V = len(m.validators.weights)
    has = fm.evidence_all(m)[0] != fm.NONE
    assert np.array_equal(hb_mark[:, :V], has)               # column c is creator c's original branch
    for c, bs in br.of_creator.items():
        assert bs[0] == c
        for b in bs[1:]:                                     # a fork branch: marked with the creator, where the row
            known = np.arange(m.n) >= br.events[b][0]        # is long enough to hold it
            assert np.array_equal(hb_mark[known, b], has[known, c])
            assert not hb_mark[~known, b].any()
    assert np.array_equal(_merged_marks(m), has)
    return has


@pytest.fixture(scope="module")
def models():
    return {s: am.Model(*am.build_shape(s)) for s in FORK_SHAPES}


def test_the_fork_shapes_are_the_quoted_ones():
    assert FORK_SHAPES == list(QUOTED)


@pytest.mark.parametrize("shape", FORK_SHAPES)
def test_evidence_is_where_the_reference_marks(models, shape):
    m = models[shape]
    has = _marks_equal_evidence(m)
    pairs, triple = QUOTED[shape]
    assert int(has.sum()) == pairs
    assert (fm.max_slot(m) >= 3) == triple
    x, y, s = fm.evidence_all(m)
    assert (x[has] < y[has]).all() and (s[has] > 0).all()
    assert (y[~has] == fm.NONE).all() and (s[~has] == 0).all()
    cr, sq = np.asarray(m.creator), np.asarray(m.seq)
    assert (cr[x[has]] == np.nonzero(has)[1]).all() and (cr[y[has]] == cr[x[has]]).all()
    assert (sq[x[has]] == s[has]).all() and (sq[y[has]] == s[has]).all()


@pytest.mark.parametrize("shape", FORK_SHAPES)
def test_interval_rule_gives_the_canonical_pair(models, shape):
    m = models[shape]
    br = fm.Branches(m)
    cnt = fm.observed_counts(m, br)                          # asserts the predicate is monotone on every branch
    assert max(len(b) for b in br.of_creator.values()) <= 7
    V = len(m.validators.weights)
    n = 0
    for h in range(m.n):
        want = fm.evidence_row(m, h)
        for c in range(V):
            got = fm.interval_rule(br, cnt[h], c)
            assert got == want.get(c, fm.NO_EVIDENCE), (h, c)
            assert fm.sweep_rule(br, cnt[h], c) == (got[2] or None)
            n += got != fm.NO_EVIDENCE
    assert n == QUOTED[shape][0]


@pytest.mark.parametrize("shape", [s for s, _ in am.BLOCK_SHAPES if s[3]])
def test_evidence_at_an_atropos_names_the_block_cheaters(shape):
    validators, events = am.build_shape(shape)
    m = am.Model(validators, events)
    blocks = am.oracle_blocks(validators, events)
    seen = 0
    for _, atropos, cheaters, _ in blocks:
        got = fm.cheaters(m, atropos)
        assert [c for c, _, _, _ in got] == sorted(int(c) for c in cheaters)
        seen += len(got)
    assert seen > 0


@pytest.mark.parametrize("name", list(fd.DAGS))
def test_directed_dags(name):
    d = fd.DAGS[name]()
    m = am.Model(d.validators, d.events)
    assert [int(c) for c in m.creator] == [e.creator - 1 for e in d.events]
    br = fm.Branches(m)
    cnt = fm.observed_counts(m, br)
    assert any(w != fm.NO_EVIDENCE for _, _, w in d.cases) and any(w == fm.NO_EVIDENCE for _, _, w in d.cases)
    for head, creator, want in d.cases:
        assert fm.evidence(m, head, creator) == want, (head, creator)
        assert fm.interval_rule(br, cnt[head], creator) == want, (head, creator)
    for h in range(m.n):                                     # and every other head
        want = fm.evidence_row(m, h)
        for c in range(d.V):
            assert fm.interval_rule(br, cnt[h], c) == want.get(c, fm.NO_EVIDENCE), (h, c)
    _marks_equal_evidence(m)


def test_directed_dag_shapes():
    """What the DAGs are for: 70 branches of one creator, a branch table past
    256 seqs, a slot of three, a fork of a fork."""
    m = am.Model(fd.many().validators, fd.many().events)
    assert len(fm.Branches(m).of_creator[0]) == fd.MANY
    d = fd.long_chain()
    assert max(e.seq for e in d.events) == 300 and d.cases[2][2][2] == 257
    assert fm.max_slot(am.Model(fd.triple().validators, fd.triple().events)) == 3
    d = fd.nested()
    br = fm.Branches(am.Model(d.validators, d.events))
    assert sorted(br.first[b] for b in br.of_creator[0]) == [1, 3, 5]
