"""From the oracle alone: the cases of tests/build_cases.py are what
tests/test_gpu_build_frames.py needs of them."""

import numpy as np
import pytest

import build_cases as bc
from oracle import corc


@pytest.mark.parametrize("V", [63, 65, 257])
def test_light_oracle_equals_the_abft_restatement(V):
    """calcFrameIdx over the index oracle (no elections) gives the frames, the
    root lists and the Build answers of the C abft restatement."""
    d = bc.star_dag(V)
    light, full = bc.Ref(d, light=True), bc.Ref(d)
    for upto in bc.checkpoints(len(d)):
        light.advance(upto)
        full.advance(upto)
        assert np.array_equal(light.frames[:upto], full.frames[:upto])
        for f in range(1, int(full.frames.max()) + 2):
            assert list(full.abo.frame_roots(f)) == light.roots.get(f, [])
        cands = light.tip_candidates([0, 3], only={0, 1, 62, 63, 64, V // 2, V - 1})
        a, b = light.answers(cands), full.answers(cands)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # frames advance within three events per validator; some candidates are roots, some not
    assert int(full.frames.max()) == 3
    f, r = full.answers(full.tip_candidates([0, 3]))
    assert len(set(map(int, f))) >= 2 and 0 < int(r.sum()) < len(r)


def test_silent_validator_reaches_the_cap():
    d = bc.silent_dag(150)
    ref = bc.Ref(d)
    ref.advance(len(d))
    assert int(ref.frames.max()) >= 111 and int(ref.frames[0]) == 1
    _, last_of = ref.tips()
    silent = bc.Cand(0, 2, [0] + [last_of[v] for v in (1, 2, 3)])
    assert ref.build(silent) == 101                          # selfParentFrame + 100
    early = bc.Ref(d)
    n40 = int(np.argmax(ref.frames >= 40)) + 1
    early.advance(n40)
    _, last_of = early.tips()
    assert early.build(bc.Cand(0, 2, [0] + [last_of[v] for v in (1, 2, 3)])) == 40 == int(early.frames[:n40].max())


def test_fork_edge_has_67_branches():
    d = bc.shape_dag((58, 6, 4, 5, 3, 3))
    o = corc.OracleIndex(d.weights)
    assert o.add_batch(d.creator, d.seq, d.poff, d.par) == -1
    assert o.num_branches() == 67


def test_tip_candidates_cover_every_branch():
    shape = (24, 30, 6, 5, 6, 2)
    d = bc.shape_dag(shape)
    ref = bc.Ref(d)
    ref.advance(len(d) // 2)
    by_branch, last_of = ref.tips()
    assert len(by_branch) > len(last_of) == 24               # fork branches have tips of their own
    cands = ref.tip_candidates(bc.ks_of(shape))
    assert len(cands) == 4 * len(by_branch)
    assert {c.parents[0] for c in cands} == set(by_branch.values())
    assert {len(c.parents) for c in cands} == {1, 2, 6, 24}
    f, r = ref.answers(cands)
    assert 0 < int(r.sum()) < len(r)
