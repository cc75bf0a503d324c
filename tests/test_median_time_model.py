"""The MedianTime model (tests/median_time_model.py) on the CPU: the
hand-checked cases of the rule, and carried == derived -- times carried
through the join as vecmt does against times derived from (branch, seq) -- for
the merged times and the medians of every event of seeded fork DAGs."""

import pytest

import median_time_model as mm
from median_time_model import FORK, NONE, SEEN


@pytest.mark.parametrize("weights,entries,default,expect", [
    # half 5: 13 -> 2, 14 -> 3, 111 -> 6
    ([3, 4, 2, 1], [(SEEN, 111), (SEEN, 112), (SEEN, 13), (SEEN, 14)], 0, 111),
    # validator 1 fork-detected: honest 6, half 3: 0 -> 0, 13 -> 2, 14 -> 3
    ([3, 4, 2, 1], [(SEEN, 111), (FORK, 0), (SEEN, 13), (SEEN, 14)], 0, 14),
    ([1, 1], [(SEEN, 9), (NONE, 0)], 5, 5),
    # honest 1, half 0: the first pair in order is the cheater's (0, 0)
    ([1, 1], [(FORK, 0), (SEEN, 50)], 7, 0),
    ([5, 2, 9], [(FORK, 0), (FORK, 0), (FORK, 0)], 7, 0),
    ([1], [(SEEN, 7)], 0, 7),
])
def test_hand_cases(weights, entries, default, expect):
    assert mm.median_time(entries, weights, default) == expect
    # the array form the GPU tests compare against
    import numpy as np
    d = mm.Derived(weights)
    kind = np.array([k for k, _ in entries])
    time = np.array([t for _, t in entries], dtype=np.uint64)
    assert d.median(kind, time, default) == expect


def _run(shape, weights):
    validators, events, times = mm.build_shape(shape, weights)
    V = len(validators)
    time_of = {e.id: t for e, t in zip(events, times)}
    store = {}
    c = mm.CarriedIndex(time_of)
    c.reset(validators, store.get)
    for e in events:
        store[e.id] = e
        c.add(e)
    d = mm.derived_of(validators, events, times)
    stats = dict(fork_entries=0, fork_branch_wins=0, all_cheaters=0, honest1_median0=0)
    for i, e in enumerate(events):
        got = c.merged(e.id)
        kind, time, win = d.merged(i)
        assert [(int(k), int(t)) for k, t in zip(kind, time)] == got, (shape, i)
        stats["fork_entries"] += int((kind == FORK).sum())
        stats["fork_branch_wins"] += int(((kind == SEEN) & (win >= V)).sum())
        stats["all_cheaters"] += int((kind == FORK).all())
        honest = sum(w for w, k in zip(validators.weights, kind) if k != FORK)
        for dflt in mm.DEFAULTS:
            m = mm.median_time(got, validators.weights, dflt)
            assert d.median(kind, time, dflt) == m, (shape, i, dflt)
            if honest == 1 and m == 0 and dflt == mm.DEFAULTS[0]:
                stats["honest1_median0"] += 1
    return stats


@pytest.mark.parametrize("shape", mm.SHAPES)
def test_carried_equals_derived(shape):
    s = _run(shape, None)
    # the inputs exercise the cases
    if shape == (12, 30, 4, 3, 5, 2):
        assert s["fork_entries"] >= 1
    if shape in ((9, 20, 3, 9, 4, 7), (40, 12, 6, 8, 4, 3)):
        assert s["fork_branch_wins"] >= 1
    if shape == (9, 20, 3, 9, 4, 7):
        assert s["all_cheaters"] >= 1


def test_honest_weight_one_gives_zero():
    """All weights 1 on the all-cheaters shape: events that still see one
    honest validator have half = 0 and return the cheaters' zero."""
    s = _run((9, 20, 3, 9, 4, 7), [1] * 9)
    assert s["honest1_median0"] >= 1


def test_times_have_ties_and_high_values():
    t = mm.event_times(180, 7)
    assert len(set(t)) < len(t)
    assert any(x >= 1 << 63 for x in t) and any(x < 1 << 63 for x in t)
