"""The election's vote kernels (k_vote_init, k_vote_round1, k_vote_round of
lx_abft_kernels.hip, through lx::launch_votes and lx::launch_votes_multi)
against tests/vote_model.py, word for word: every votes table, the decision
words and the error word.  The observe relation goes to the kernels as the
per-voter bitmaps they read (tests/csrc/vote_harness.cpp), so the reference's
own election cases -- a fake relation no DAG realises -- and directed sums,
errors and sizes reach them.  tests/test_vote_model.py pins the model to the
restatement of election_math.go.

What the directed cases settled:

* An observed slot of the frame before whose event is LX_NONE is not a missing
  vote: k_vote_init writes "voted no" into every row of the launch, the round
  kernels only skip such a slot as a voter.  kVoteErrMissing needs a slot the
  launches never covered (a slot range that stops before it).
* The kernels check every slot against every subject of the window; the
  reference stops asking about a subject once it is decided and stops the
  election once the Atropos is known.  test_younger_slot_trips_check: a slot
  younger than the decision that observes less than the quorum sets
  kVoteErrQuorum although the decision words hold the reference's decision;
  check_decision reads the error word first.

Measured on an MI355X: test_random_relations[130] 0.26 s, [65] 0.10 s,
test_wide_stride_loop 0.11 s, test_wide_windows 0.07 s (the 2100-slot
fixture is built once, 0.05 s), every other case 0.01 s or less but for the
first to load the library (0.24 s).  The module in 1.3 s.
"""

import ctypes
import json
import os

import numpy as np
import pytest

import vote_model as vm

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
u32p = ctypes.POINTER(ctypes.c_uint32)
u64p = ctypes.POINTER(ctypes.c_uint64)
ALL = 1 << 30
_lib = None


def lib():
    global _lib
    if _lib is None:
        L = ctypes.CDLL(os.path.join(os.path.dirname(HERE), "lachesis-base_amd", "build", "libvote_harness.so"))
        L.vh_last_error.restype = ctypes.c_char_p
        L.vh_run.argtypes = [ctypes.c_uint32, u32p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, u32p, u32p, u32p,
                             u32p, u64p, u32p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, u32p, ctypes.c_uint32,
                             u32p, ctypes.c_uint64, u64p, u32p]
        _lib = L
    return _lib


def device_run(rel, E=1, stride=None, steps=None, merged=False, rc_want=0, pad_ones=False):
    """vote_model.run on the GPU.  pad_ones: the bits of a bitmap's last word
    past its length are set (the kernels must not read them as roots)."""
    stride = rel.V if stride is None else stride
    steps = [(0, stride, 0, ALL)] if steps is None else steps
    p = lambda a, t: a.ctypes.data_as(t)
    slot_off = np.cumsum([0] + [len(x) for x in rel.ev]).astype(np.uint32)
    ev = np.concatenate(rel.ev).astype(np.uint32)
    creator = np.concatenate(rel.creator).astype(np.uint32)
    dup = np.concatenate(rel.dup).astype(np.uint32)
    bm_off, words = [], []
    for o in rel.obs:
        nw = (o.shape[1] + 31) // 32
        bits = np.zeros((o.shape[0], nw * 32), dtype=np.uint8)
        bits[:, :o.shape[1]] = o
        if pad_ones:
            bits[:, o.shape[1]:] = 1
        packed = np.packbits(bits, axis=1, bitorder="little").view(np.uint32).reshape(o.shape[0], nw)
        base = sum(len(x) for x in words)
        bm_off += [base + i * nw for i in range(o.shape[0])]
        words.append(packed.ravel())
    bm = np.concatenate(words + [np.zeros(1, dtype=np.uint32)]).astype(np.uint32)
    bm_off = np.array(bm_off, dtype=np.uint64)
    order, off, tot = vm.tables(rel, E, stride)
    st = np.array(steps, dtype=np.uint32).reshape(-1, 4)
    w = rel.w.astype(np.uint32)
    votes = np.zeros(max(tot, 1), dtype=np.uint32)
    dec = np.zeros((E, stride), dtype=np.uint64)
    err = np.zeros(E, dtype=np.uint32)
    rc = lib().vh_run(rel.V, p(w, u32p), rel.quorum, rel.G, E, p(slot_off, u32p), p(ev, u32p), p(creator, u32p),
                      p(dup, u32p), p(bm_off, u64p), p(bm, u32p), len(bm), stride, len(st), p(st, u32p), int(merged),
                      p(votes, u32p), tot, p(dec, u64p), p(err, u32p))
    assert rc == rc_want, lib().vh_last_error()
    tabs = {ek: votes[off[ek]:off[ek] + len(rel.ev[ek[1]]) * stride].reshape(-1, stride).astype(np.int64) for ek in order}
    return tabs, dec, err


def assert_same(rel, votes=True, pad_ones=False, **kw):
    """Device == model; returns the device's result."""
    want = vm.run(rel, **kw)
    got = device_run(rel, pad_ones=pad_ones, **kw)
    assert got[2].tolist() == want[2].tolist(), "error words"
    if votes:
        for ek in want[0]:
            bad = np.argwhere(got[0][ek] != want[0][ek])
            assert not len(bad), (ek, bad[:4].tolist())
        assert np.array_equal(got[1], want[1]), "decision words"
    return got


# ---------------------------------------------------------------------------- the reference's election cases

@pytest.fixture(scope="module")
def cases():
    with open(os.path.join(HERE, "golden", "abft_golden.json"), encoding="utf-8") as f:
        return json.load(f)["election_cases"]


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4, 5])
def test_election_cases(cases, seed):
    decided = 0
    for c in cases:
        case = vm.golden_case(c, seed)
        rel = vm.relation_of(*case)
        for merged in (False, True):
            _, dec, _ = assert_same(rel, merged=merged)
            state = vm.atropos_state(dec[0])
            exp = c["expected"]
            if exp is None:
                assert state == ("pending",)
                continue
            names = [e.name.lstrip("+") for e in case[1]]
            frame0 = [i for i, e in enumerate(case[1]) if case[2][e.id] == 0]
            _, res, at = vm.reference_election(*case)
            assert state[0] == "decided" and exp["frame"] == 0
            assert names[frame0[state[2]]] == exp["atropos"]          # the Atropos
            assert names[state[1]] in exp["decisive"] and state[1] == at   # the first decisive root
            decided += 1
    assert decided == 8
    assert sum(cases[3]["weights"].values()) == 2**31 - 1    # "differentWeights": the largest total the sums hold


# ---------------------------------------------------------------------------- random relations

@pytest.mark.parametrize("V", [4, 7, 65, 130])
def test_random_relations(V):
    short = False
    for seed in range(3):
        rel = vm.relation_of(*vm.random_case(V, 100 * V + seed))
        short |= any(len(e) < V for e in rel.ev)               # some validators without a root in a frame
        _, _, err = assert_same(rel)
        assert err[0] == 0
        # as run_elections_ahead lays them out: elections of frames 0..2, window min(V, 64)
        _, _, err = assert_same(rel, E=3, stride=min(V, 64), merged=True)
        assert not err.any()
        assert_same(rel, E=3, stride=min(V, 64), merged=False)
    assert short


# ---------------------------------------------------------------------------- directed sums

def three_frames(w, sees0, observed, quorum=None):
    """Frame 0: one root per validator.  Frame 1: one root per validator,
    slot i observing root 0 iff sees0[i] and every other root.  Frame 2: one
    slot per entry of ``observed`` (the frame-1 slots it observes).  For
    subject 0 a frame-2 slot then sums yes = the stake of its observed slots
    with sees0, no = the stake of the others."""
    V = len(w)
    rel = vm.Relation(w, quorum)
    rel.add_frame(range(V), range(V))
    o1 = np.ones((V, V), dtype=bool)
    o1[:, 0] = sees0
    rel.add_frame(range(V, 2 * V), range(V), o1)
    o2 = np.zeros((len(observed), V), dtype=bool)
    for s, rs in enumerate(observed):
        o2[s, rs] = True
    rel.add_frame(range(2 * V, 2 * V + len(observed)), range(len(observed)), o2)
    return rel


Y0 = vm.VOTED | vm.YES | 0          # yes, names root slot 0
N = vm.VOTED | vm.NOROOT            # no
D = vm.DECIDED

SUMS = [
    # weights, sees0, observed frame-1 slots, word for subject 0, error word
    ("tie_equal", [1, 1, 1, 1], [1, 1, 0, 0], [0, 1, 2, 3], Y0, 0),              # yes 2 = no 2: yes, not decided
    ("tie_unequal", [3, 1, 1, 1], [1, 0, 0, 0], [0, 1, 2, 3], Y0, 0),            # yes 3 = no 3
    ("tie_unequal_big", [2**30 - 2, 2**29, 2**29 - 1, 1], [1, 0, 0, 1], [0, 1, 2, 3], Y0, 0),   # 2^30 - 1 each
    ("yes_quorum", [1, 1, 1, 1], [1, 1, 1, 0], [0, 1, 2, 3], Y0 | D, 0),         # yes 3 = quorum
    ("yes_quorum_less_1", [1, 1, 1, 1], [1, 1, 0, 0], [0, 1, 2], Y0, 0),         # yes 2, no 1
    ("no_quorum", [1, 1, 1, 1], [0, 0, 0, 1], [0, 1, 2, 3], N | D, 0),           # no 3 = quorum
    ("no_quorum_less_1", [1, 1, 1, 1], [0, 0, 1, 1], [0, 1, 2], N, 0),           # no 2, yes 1
    ("yes_quorum_w", [5, 4, 3, 2, 1], [1, 1, 0, 1, 0], [0, 1, 2, 3, 4], Y0 | D, 0),   # yes 11 = quorum of 15
    ("yes_quorum_w_less_1", [5, 4, 3, 2, 1], [1, 1, 0, 0, 1], [0, 1, 2, 3, 4], Y0, 0),   # yes 10, no 5
    ("no_quorum_w", [5, 4, 3, 2, 1], [0, 0, 0, 1, 1], [0, 1, 2, 3], N | D, 0),   # no 12 > quorum 11, yes 2
    ("no_quorum_w_exact", [5, 4, 3, 2, 1], [0, 0, 1, 0, 1], [0, 1, 2, 3, 4], N | D, 0),   # no 11 = quorum, yes 4
    ("no_quorum_w_less_1", [5, 4, 3, 2, 1], [0, 1, 0, 0, 0], [0, 1, 2, 3], N, 0),   # no 10, yes 4
    ("all_quorum", [1, 1, 1, 1], [1, 1, 1, 1], [1, 2, 3], Y0 | D, 0),            # all 3 = quorum: no error
    ("all_quorum_less_1", [1, 1, 1, 1], [1, 1, 1, 1], [2, 3], Y0, vm.ERR_QUORUM),   # all 2
    ("all_quorum_w", [5, 4, 3, 2, 1], [1, 1, 1, 1, 1], [0, 1, 3], Y0 | D, 0),    # all 11 = quorum
    ("all_quorum_w_less_1", [5, 4, 3, 2, 1], [1, 1, 1, 1, 1], [0, 1, 4], Y0, vm.ERR_QUORUM),   # all 10
]


@pytest.mark.parametrize("name,w,sees0,observed,word,err", SUMS, ids=[s[0] for s in SUMS])
def test_directed_sums(name, w, sees0, observed, word, err):
    rel = three_frames(w, sees0, [observed])
    for merged in (False, True):
        votes, dec, e = assert_same(rel, merged=merged)
        assert int(votes[(0, 2)][0, 0]) == word
        assert int(e[0]) == err
        want = (int(rel.ev[2][0]) << 32) | (0x80000000 if word & vm.YES else 0) | (word & vm.NOROOT)
        assert int(dec[0][0]) == (want if word & D else vm.UNDECIDED)


# ---------------------------------------------------------------------------- directed errors

def test_missing_vote():
    """Frame-1 slots [2, 4) are never voted (the step's slot range stops at
    2), the frame-2 slot observes slot 3."""
    rel = three_frames([1, 1, 1, 1], [1, 1, 1, 1], [[0, 1, 3]])
    _, _, err = assert_same(rel, steps=[(0, 4, 0, 2)])
    assert err[0] == vm.ERR_MISSING
    _, _, err = assert_same(rel, steps=[(0, 4, 0, 4)])
    assert err[0] == 0


def test_none_slot_observed_is_a_no_vote():
    """A frame-1 slot without an event: skipped as a voter, its row is what
    k_vote_init wrote (voted no), no kVoteErrMissing."""
    rel = three_frames([1, 1, 1, 1], [1, 1, 1, 1], [[0, 1, 2, 3]])
    rel.ev[1][3] = vm.NONE
    votes, _, err = assert_same(rel)
    assert err[0] == 0 and (votes[(0, 1)][3] == N).all()
    assert int(votes[(0, 2)][0, 0]) == Y0 | D                 # yes 3, no 1


def test_two_roots_of_one_validator():
    """prev_dup: frame 1 holds two slots of validator 0, the frame-2 slot
    observes both (allVotes.Count fails in the reference)."""
    V = 4
    rel = vm.Relation([1] * V)
    rel.add_frame(range(V), range(V))
    rel.add_frame(range(V, 2 * V + 1), [0, 1, 2, 3, 0], np.ones((V + 1, V), dtype=bool))
    assert rel.dup[1].tolist() == [vm.NONE] * 4 + [0]
    for observed, err in (([0, 1, 2, 4], vm.ERR_TWO_ROOTS), ([1, 2, 3, 4], 0), ([0, 1, 2, 3], 0)):
        o = np.zeros((1, V + 1), dtype=bool)
        o[0, observed] = True
        r2 = vm.Relation(rel.w)
        r2.ev, r2.creator, r2.dup, r2.obs = list(rel.ev), list(rel.creator), list(rel.dup), list(rel.obs)
        r2.add_frame([20], [0], o)
        for merged in (False, True):
            _, _, e = assert_same(r2, votes=err == 0, merged=merged)
            assert e[0] == err


@pytest.mark.parametrize("second,form", [(4, "one wave slice"), (1, "across slices")])
def test_two_yes_votes_name_different_roots(second, form):
    """Frame 0 holds two roots of validator 0 (slots 0 and 5).  Frame-1 slot
    0 observes the first, slot ``second`` the other, the rest neither; the
    frame-2 slot observes slots 0..4 of frame 1.  All five sit in one bitmap
    word, so they are compacted in slot order and observed root k goes to wave
    slice k % 4: slots 0 and 4 meet inside slice 0, slots 0 and 1 only when
    the slices' tallies are merged."""
    V = 5
    rel = vm.Relation([1] * V)
    rel.add_frame(range(6), [0, 1, 2, 3, 4, 0])
    o1 = np.ones((V, 6), dtype=bool)
    o1[:, [0, 5]] = False
    o1[0, 0] = True
    o1[second, 5] = True
    rel.add_frame(range(6, 6 + V), range(V), o1)
    rel.add_frame([11], [0], np.ones((1, V), dtype=bool))
    for merged in (False, True):
        votes, _, err = assert_same(rel, votes=False, merged=merged)
        assert int(votes[(0, 1)][0, 0]) == Y0 and int(votes[(0, 1)][second, 0]) == vm.VOTED | vm.YES | 5
        assert err[0] == vm.ERR_TWO_ROOTS
    # the same with both naming slot 0: no error
    o1[second, 5], o1[second, 0] = False, True
    rel.obs[1] = o1
    _, _, err = assert_same(rel)
    assert err[0] == 0


def test_younger_slot_trips_check():
    """Frame 2 decides every subject at its slot 0 (event 8); slot 1 (event 9,
    younger than the decision) observes only 2 of 4.  The reference returns
    its decision at event 8 and never asks event 9; the kernels set
    kVoteErrQuorum next to the same decision words."""
    rel = three_frames([1, 1, 1, 1], [1, 1, 1, 1], [[0, 1, 2, 3], [2, 3]])
    _, dec, err = assert_same(rel)
    assert vm.atropos_state(dec[0]) == ("decided", 8, 0)
    assert err[0] == vm.ERR_QUORUM
    older_only = three_frames([1, 1, 1, 1], [1, 1, 1, 1], [[0, 1, 2, 3]])
    _, dec, err = assert_same(older_only)
    assert vm.atropos_state(dec[0]) == ("decided", 8, 0) and err[0] == 0


# ---------------------------------------------------------------------------- sizes

@pytest.fixture(scope="module")
def wide():
    """V 2100, frames 0 and 1 with 2100 slots, frame 2 with 70: its bitmaps
    take two kObsChunk = 2048 passes, the second of 52 bits.  Roots 0..9 of
    frame 0 are observed by every frame-1 slot (decided yes), roots 10..19 by
    none (decided no), the rest by ~3/4; every frame-2 slot observes ~3/4 of
    frame 1 and bits on both sides of 2048."""
    V, rng = 2100, np.random.default_rng(2100)
    rel = vm.Relation([1] * V)
    rel.add_frame(range(V), rng.permutation(V))
    o1 = rng.random((V, V)) < 0.75
    o1[:, np.isin(rel.creator[0], np.arange(10))] = True
    o1[:, np.isin(rel.creator[0], np.arange(10, 20))] = False
    # subject 20 at the edge: frame-1 slots [0, 1400) vote no on it, slot 0 of
    # frame 2 observes exactly those and four more -- no = 1400 = quorum - 1,
    # so one root too many (or too few) in its sums changes its vote word
    o1[:1400, rel.creator[0] == 20] = False
    o1[1400:, rel.creator[0] == 20] = True
    rel.add_frame(range(V, 2 * V), rng.permutation(V), o1)
    o2 = rng.random((70, V)) < 0.75
    o2[0] = np.arange(V) < 1400
    o2[:, [2047, 2048, 2099]] = True
    o2[::2, 2079] = True            # word 64 of the row: bits 2048..2099 valid
    rel.add_frame(range(2 * V, 2 * V + 70), rng.permutation(V)[:70], o2)
    assert o2.sum(axis=1).min() >= rel.quorum == 1401 and o2[0].sum() == 1404
    return rel


def test_wide_windows(wide):
    first, dec1, _ = assert_same(wide, steps=[(0, 64, 0, ALL)])
    both, dec2, err = assert_same(wide, steps=[(0, 64, 0, ALL), (64, 128, 0, ALL)])
    assert err[0] == 0
    for ek in first:
        assert np.array_equal(both[ek][:, :64], first[ek][:, :64])       # [64, 128) left [0, 64) alone
        assert not both[ek][:, 128:].any() and both[ek][:, 64:128].all()  # and nothing past it
    assert np.array_equal(dec2[0][:64], dec1[0][:64]) and (dec2[0][128:] == vm.UNDECIDED).all()
    yes = (dec2[0][:20] & np.uint64(0x80000000)) != 0
    assert yes[:10].all() and not yes[10:].any() and (dec2[0][:20] != vm.UNDECIDED).all()


def test_wide_stride_loop(wide):
    """[0, 1100): 18 chunks of 64 subjects over 16 workgroups per slot."""
    votes, dec, err = assert_same(wide, steps=[(0, 1100, 0, ALL)])
    assert err[0] == 0 and not votes[(0, 2)][:, 1100:].any()


def test_wide_bits_past_the_length_are_ignored(wide):
    """bm_len = 2100 leaves 12 bits of each row's last word unused: set, they
    are masked off by the second compaction pass (the engine's rows hold zeros
    there; with the 70 slots of frame 2 behind frame 1's in every array of the
    harness, reading them as roots 2100..2111 would still stay inside it)."""
    assert len(wide.ev[1]) % 32 == 20 and len(wide.ev[2]) >= 12
    votes, _, err = assert_same(wide, steps=[(0, 64, 0, ALL)], pad_ones=True)
    assert err[0] == 0
    assert int(votes[(0, 2)][0, 20]) == N          # no 1400 = quorum - 1, yes 4: not decided


# ---------------------------------------------------------------------------- launch_votes_multi

def test_multi_unequal_tables():
    """Elections of frames 0, 1, 2 over frames of 80 / 3 / 70 / 5 / 70 slots
    (one of the 5 without an event): the round-1 launch holds tables of 3, 70
    and 5 voters, every later launch tables of unequal size too; each election
    has its own decision and error words."""
    V, rng = 80, np.random.default_rng(80)
    rel = vm.Relation([1000] * 3 + [1] * 77)
    prev = None
    for k, n in enumerate([80, 3, 70, 5, 70]):
        creators = np.concatenate([np.arange(3), 3 + rng.permutation(77)[:n - 3]])[rng.permutation(n)]
        obs = None
        if prev is not None:
            obs = rng.random((n, len(prev))) < 0.6
            obs[:, prev < 3] = True                     # the heavy three: 3000 of quorum 2052
        rel.add_frame(100 * k + np.arange(n), creators, obs)
        prev = creators
    light = int(np.nonzero(rel.creator[3] >= 3)[0][0])
    rel.ev[3][light] = vm.NONE
    votes, dec, err = assert_same(rel, E=3, stride=64, merged=True)
    assert not err.any()
    assert (votes[(0, 3)][light] == N).all() and (votes[(2, 3)][light] == N).all()
    states = [vm.atropos_state(dec[e]) for e in range(3)]
    assert [s[0] for s in states] == ["decided"] * 3 and len({s[1] for s in states}) == 3
    single = device_run(rel, E=3, stride=64, merged=False)
    for ek in votes:
        assert np.array_equal(single[0][ek], votes[ek])
    assert np.array_equal(single[1], dec)


def test_harness_refuses_malformed_input():
    """Every index is checked on the host; nothing is launched."""
    rel = three_frames([1, 1, 1, 1], [1, 1, 1, 1], [[0, 1, 2, 3]])
    rel.creator[1] = rel.creator[1].copy()
    rel.creator[1][2] = 4
    device_run(rel, rc_want=-1)
    rel.creator[1][2] = 2
    device_run(rel, steps=[(0, 5, 0, ALL)], rc_want=-1)
    device_run(rel, stride=5, rc_want=-1)
    rel.dup[1] = rel.dup[1].copy()
    rel.dup[1][1] = 3
    device_run(rel, rc_want=-1)
