"""Pin tests/vote_model.py (the reference the vote kernels are compared with,
tests/test_gpu_votes.py) to oracle.abft_oracle.Election, the restatement of
election_math.go that tests/test_abft_oracle.py pins to the reference's own
election tests.  CPU only.

The roots are processed in event-id order.  Election asks a root only about
subjects not decided yet and stops at the Atropos, the model answers every
subject for every slot: every vote Election recorded equals the model's word,
every decision Election recorded is the model's decision word (the minimum
over the deciding events: the first one), and chooseAtropos over the model's
decision words in idx order -- restated in vote_model.atropos_state, with the
event at which the last needed subject was decided -- is Election's answer at
the root where it first gave one.
"""

import json
import os

import pytest

import vote_model as vm
from oracle import abft_oracle as ao

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def cases():
    with open(os.path.join(HERE, "golden", "abft_golden.json"), encoding="utf-8") as f:
        return json.load(f)["election_cases"]


def check_against_election(case):
    validators, order, frame_of, edges = case
    rel = vm.relation_of(*case)
    votes, dec, err = vm.run(rel)
    pos_of = {e.id: i for i, e in enumerate(order)}
    slot_of = {e.id: (frame_of[e.id], s) for k in range(rel.G + 1)
               for s, e in enumerate(x for x in order if frame_of[x.id] == k)}
    try:
        el, res, at = vm.reference_election(*case)
    except ao.ElectionError as ex:
        assert "all the roots are decided as 'no'" in str(ex)
        assert vm.atropos_state(dec[0]) == ("all_no",)
        return None, rel, dec

    def same(vote, word):
        assert word & vm.VOTED
        assert bool(word & vm.YES) == vote.yes and bool(word & vm.DECIDED) == vote.decided
        want = vm.NOROOT if vote.observed_root is None else slot_of[vote.observed_root][1]
        assert word & vm.NOROOT == want

    assert el.votes
    for (root, subject), vote in el.votes.items():
        k, s = slot_of[root.id]
        same(vote, int(votes[(0, k)][s, validators.idxs[subject]]))
    for subject, vote in el.decided_roots.items():
        word = int(dec[0][validators.idxs[subject]])
        assert word != vm.UNDECIDED
        k, s = slot_of[order[word >> 32].id]
        same(vote, int(votes[(0, k)][s, validators.idxs[subject]]))
        assert bool(word & 0x80000000) == vote.yes
    state = vm.atropos_state(dec[0])
    if res is None:
        assert state == ("pending",)
    else:
        assert state == ("decided", at, slot_of[res[1]][1]) and res[0] == 0
    return res, rel, dec


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4, 5])
def test_model_matches_election_golden(cases, seed):
    decided = 0
    for c in cases:
        case = vm.golden_case(c, seed)
        res, rel, dec = check_against_election(case)
        exp = c["expected"]
        assert (res is None) == (exp is None)
        if exp is not None:
            decided += 1
            names = {e.id: e.name.lstrip("+") for e in case[1]}
            _, at, _ = vm.atropos_state(dec[0])
            assert names[res[1]] == exp["atropos"] and names[case[1][at].id] in exp["decisive"]
    assert decided == 4


@pytest.mark.parametrize("V", [4, 7, 65, 130])
def test_model_matches_election_random(V):
    n = 0
    for seed in range(6 if V < 65 else 2):
        res, rel, dec = check_against_election(vm.random_case(V, 100 * V + seed))
        assert int(vm.run(rel)[2][0]) == 0       # error-free by construction
        n += res is not None
    assert n >= 1


def test_model_windows_and_slot_ranges():
    """Steps over subject windows (each over every frame, as widen_window
    goes) give the table of one launch and leave the rest of it alone; a slot
    range that leaves observed slots of the frame before without a vote is the
    reference's "every root must vote" error."""
    rel = vm.relation_of(*vm.random_case(130, 7))
    whole = vm.run(rel)
    parts = vm.run(rel, steps=[(0, 64, 0, 1 << 30), (64, 128, 0, 1 << 30), (128, 130, 0, 1 << 30)])
    for ek in whole[0]:
        assert (whole[0][ek] == parts[0][ek]).all()
    assert (whole[1] == parts[1]).all() and whole[2][0] == 0 and parts[2][0] == 0
    first = vm.run(rel, steps=[(0, 64, 0, 1 << 30)])
    for ek in whole[0]:
        assert (first[0][ek][:, :64] == whole[0][ek][:, :64]).all() and not first[0][ek][:, 64:].any()
    assert min(len(x) for x in rel.ev) > 50 and all(o[:, 50:].any() for o in rel.obs[2:])
    assert vm.run(rel, steps=[(0, 130, 0, 50)])[2][0] == vm.ERR_MISSING
