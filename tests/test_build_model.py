"""The rule lx_abft_build_frames rests on (tests/build_model.py), on the CPU: at
several points of an epoch, the frame the model gives a candidate that is not
added -- virtual HighestBefore row, own-creator term, frame loop over the
engine's roots -- equals oracle.abft_oracle IndexedLachesis.build(e), which
adds the event, asks, and drops it."""

import pytest

import build_model as bm


def checkpoints(n):
    return sorted({max(1, n // 5), max(1, n // 2), n})


def check_epoch(ep, P):
    """Every tip candidate at every checkpoint; returns what the two hard
    parts did: (candidates, rows that gained a mark no parent carries,
    ForklessCause answers the own-creator correction changed)."""
    V = len(ep.validators)
    n_cand = new_marks = fc_changed = 0
    for upto in checkpoints(len(ep.events)):
        ep.advance(upto)
        m = bm.Model(ep)
        for c in ep.tip_candidates(sorted({0, 1, max(P - 1, 0), V - 1})):
            assert m.refusal(c) is None and not ep.opens_branch(c)
            spf, f = m.frame(c)
            assert f == ep.oracle_frame(c), (upto, c.tip, c.k)
            assert spf <= f <= spf + bm.BUILD_CAP
            n_cand += 1
            row = m.virtual_row(c)
            new_marks += bool((row[1] & ~row[2]).any())
            for fr in range(spf, f + 1):
                for r in m.roots.get(fr, []):
                    fc_changed += m.forkless_cause(c, row, r) != m.forkless_cause(c, row, r, corrected=False)
        # the refused candidates are exactly the ones that would open a branch
        for c in ep.off_tip_candidates():
            assert (m.refusal(c) == "branch") == ep.opens_branch(c)
            assert m.refusal(c) in ("branch", None)
    return n_cand, new_marks, fc_changed


@pytest.mark.parametrize("shape", bm.SHAPES)
def test_model_frame_equals_oracle_build(shape):
    ep = bm.Epoch.of_shape(shape)
    n_cand, new_marks, fc_changed = check_epoch(ep, shape[2])
    assert n_cand >= 3 * min(shape[0], 4)
    # The two hard parts are exercised.  The correction changes a ForklessCause
    # answer where a root is an ancestor through other parents only (never with
    # V = 1: every LA(r)[0] is set; not at the checkpoints of the 12-validator
    # fork shape, measured: 0).  Rule (ii): a candidate joins two branches of a
    # cheater that none of its parents saw together.
    if shape in ((3, 12, 3, 0, 0, 2), (16, 40, 5, 0, 0, 1), (24, 30, 6, 5, 6, 2)):
        assert fc_changed > 0
    assert (new_marks > 0) == (shape[3] > 0)


def test_own_stake_decides():
    """Weights [5, 2, 2]: the quorum is 7, so no quorum forms without the
    heavy validator -- its candidates pass only by their own stake."""
    ep = bm.Epoch.of_shape((3, 12, 3, 0, 0, 2), weights=[5, 2, 2])
    assert ep.validators.quorum() == 7
    n_cand, _, fc_changed = check_epoch(ep, 3)
    assert n_cand and fc_changed > 0
    m = bm.Model(ep)
    heavy = [c for c in ep.tip_candidates([2]) if c.creator == 0]
    assert heavy
    for c in heavy:
        spf, f = m.frame(c)
        assert f == ep.oracle_frame(c)
        # without the correction the candidate's own 5 of 9 are missing wherever
        # its self-parent is no ancestor of the root: the frame can only fall
        assert m.frame(c, corrected=False)[1] <= f


def test_uncorrected_rule_is_wrong_somewhere():
    """The check has teeth: dropping the own-creator correction changes a frame."""
    ep = bm.Epoch.of_shape((3, 12, 3, 0, 0, 2), weights=[5, 2, 2])
    ep.advance(len(ep.events))
    m = bm.Model(ep)
    cands = ep.tip_candidates([0, 1, 2])
    assert any(m.frame(c, corrected=False)[1] != ep.oracle_frame(c) for c in cands)
    assert all(m.frame(c)[1] == ep.oracle_frame(c) for c in cands)
