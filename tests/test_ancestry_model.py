"""What the ancestry kernels rest on (tests/ancestry_model.py), on the CPU: for
every pair of seeded fork DAGs the LowestAfter rule equals the walk, the
HighestBefore rule equals it wherever the entry is no fork marker, and the
marked pairs hold both answers; and the model's confirmEvents reproduces, as
sets, every block the abft oracle decides."""

import pytest

import ancestry_model as am


@pytest.mark.parametrize("shape", am.PAIR_SHAPES)
def test_rules_equal_the_walk(shape):
    validators, events = am.build_shape(shape)
    m = am.Model(validators, events)
    assert 6 <= m.n <= 771
    dfs = m.observes_matrix()
    for a in (0, m.n // 2, m.n - 1):                         # the matrix is the bitsets
        assert [bool(v) for v in dfs[a]] == [m.observes(a, x) for x in range(m.n)]
    assert dfs.diagonal().all() and not dfs[0, 1:].any()
    assert (dfs == m.la_rule_matrix()).all()
    hb, marked = m.hb_rule_matrix()
    assert (hb[~marked] == dfs[~marked]).all()
    if shape == (257, 3, 8, 5, 2, 6):
        # three events per cheater: a head that sees the fork sees all three,
        # so every one of the 1,662 marked pairs is an ancestor pair
        assert marked.sum() == 1662 and dfs[marked].all()
    elif shape[3]:                                           # cheaters: a wrong fallback would show
        assert dfs[marked].any() and not dfs[marked].all()
    else:
        assert not marked.any()


def test_marked_pairs_of_the_quoted_shape():
    """(12,30,4,3,5,2): 16,040 of the 28,648 marked pairs are ancestors."""
    m = am.Model(*am.build_shape((12, 30, 4, 3, 5, 2)))
    _, marked = m.hb_rule_matrix()
    assert (int(marked.sum()), int(m.observes_matrix()[marked].sum())) == (28648, 16040)


@pytest.mark.parametrize("shape,min_blocks", am.BLOCK_SHAPES)
def test_confirm_reproduces_the_oracle_blocks(shape, min_blocks):
    validators, events = am.build_shape(shape)
    blocks = am.oracle_blocks(validators, events)
    assert len(blocks) >= min_blocks
    m = am.Model(validators, events)
    marked = 0
    for frame, atropos, cheaters, confirmed in blocks:
        got, = m.confirm([atropos], [frame])
        assert len(set(got)) == len(got) == len(confirmed)
        assert set(got) == set(confirmed), frame
        marked += sum(int(m.creator[e]) in cheaters for e in confirmed)
        # ancestor-closed labels: the walk found every unlabelled ancestor
        assert all(m.label[e] for e in range(atropos + 1) if m.observes(atropos, e))
    if shape[3]:
        assert marked > 0
    assert m.low_water() <= m.n


def test_confirm_stops_at_labelled_events():
    """After arbitrary labels the walk and "every unlabelled ancestor" differ:
    the header promises the latter."""
    validators, events = am.build_shape((7, 25, 3, 0, 0, 1))
    a, b = am.Model(validators, events), am.Model(validators, events)
    head = a.n - 1
    cut = [e for e in a.parents[head]]
    for m in (a, b):
        for e in cut:
            m.label[e] = 9
    walk, = a.confirm([head], [5])
    every, = b.confirm_all_ancestors([head], [5])
    assert walk == [head] and len(every) > 1 and set(walk) < set(every)
