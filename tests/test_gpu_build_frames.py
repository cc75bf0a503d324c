"""lx_abft_build_frames: the frames of candidate events that are not added,
computed from the planes (k_build_rows, the OWN forms of k_root_fc /
k_root_fc16, k_root_quorum), against two yardsticks -- the oracle's Build
(tests/build_cases.py: the C abft restatement, or calcFrameIdx over the C index
oracle where elections are too slow on the CPU) and lx_abft_build called
candidate by candidate on the same handle afterwards (add, evaluate, drop).

Edges of the kernels the shapes cross: rows wider than one wave (64 columns),
than one workgroup pass of k_build_rows (256 threads x 4 columns = 1024) and
than k_root_fc's 32-column LDS chunks (V = 63, 65, 257, 1030; B = 67 with
forks); more than one 64-candidate tile and more than 256 candidates (n = 300);
candidates at different frames in one launch and more than one round (the
silent validator: 100 rounds); the 16-bit kernel's gate on the candidate's own
seq (0x10000).
"""

import functools

import numpy as np
import pytest

import build_cases as bc

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -1, -4
SHAPES = [(1, 6, 1, 0, 0, 1), (3, 12, 3, 0, 0, 2), (16, 40, 5, 0, 0, 1), (12, 30, 4, 3, 5, 2), (24, 30, 6, 5, 6, 2)]
FORK_EDGE = (58, 6, 4, 5, 3, 3)                              # B = 67: three columns past a wave


def gpu_handle(d, options=None, cls=None):
    from lachesis_hip import abft
    lch = (cls or abft.DenseLachesis)(d.weights, event_capacity=len(d) + 8)
    for k, v in (options or {}).items():
        lch.set_option(k, v)
    return lch


def feed(lch, d, lo, hi, chunk=97, claimed=None):
    """Events [lo, hi) through lx_abft_process_batch in chunks; returns their frames."""
    out = []
    for a in range(lo, hi, chunk):
        b = min(hi, a + chunk)
        c, s, off, par = d.slice(a, b)
        rc, consumed, fr = lch.process_batch(c, s, off, par, None if claimed is None else claimed[a:b])
        assert rc == 0 and consumed == b - a
        out.append(fr)
    return np.concatenate(out) if out else np.zeros(0, dtype=np.uint32)


def ask(lch, cands):
    rc, err, frames, roots = lch.build_frames(*bc.dense(cands))
    assert rc == 0, lch.L.lx_abft_last_error(lch.h).decode()
    return frames, roots


def three_way(lch, ref, cands, one_by_one=True):
    """One call, one call per candidate, the oracle's Build, lx_abft_build."""
    exp_f, exp_r = ref.answers(cands)
    f, r = ask(lch, cands)
    assert np.array_equal(f, exp_f) and np.array_equal(r, exp_r)
    if one_by_one:
        for i, c in enumerate(cands):
            f1, r1 = ask(lch, [c])
            assert (int(f1[0]), int(r1[0])) == (int(exp_f[i]), int(exp_r[i])), i
    # the parent commit's call, afterwards: add, evaluate, drop
    for i, c in enumerate(cands):
        assert lch.build(c.creator, c.seq, c.parents) == exp_f[i], i
    return exp_f, exp_r


@functools.lru_cache(maxsize=None)
def shape_dag(shape, weights=None):
    return bc.shape_dag(shape, weights)


@pytest.mark.parametrize("shape,weights", [(s, None) for s in SHAPES] + [((3, 12, 3, 0, 0, 2), (5, 2, 2))],
                         ids=lambda x: "-".join(map(str, x)) if x else "eq")
def test_tip_candidates_at_three_checkpoints(shape, weights):
    """Every branch tip x k other parents in {0, 1, P - 1, all}, early, in the
    middle and at the end of the epoch.  V = 1: every quorum rests on the
    own-creator term alone.  Weights 5, 2, 2: the candidate's own stake decides."""
    d = shape_dag(shape, weights)
    ref, lch = bc.Ref(d), gpu_handle(d)
    try:
        done, roots_seen = 0, 0
        for upto in bc.checkpoints(len(d)):
            ref.advance(upto)
            assert np.array_equal(feed(lch, d, done, upto, chunk=37), ref.frames[done:upto])
            done = upto
            cands = ref.tip_candidates(bc.ks_of(shape))
            assert len(cands) >= len(bc.ks_of(shape)) * min(shape[0], 3)
            _, r = three_way(lch, ref, cands)
            roots_seen += int(r.sum())
        assert roots_seen > 0
        if shape[3]:
            assert lch.ix.num_branches() > shape[0]
    finally:
        lch.close()


def test_many_frames_in_one_call():
    """Four equal validators, one silent after its first event while the others
    run 113 frames: its candidate on all tips climbs selfParentFrame + 100
    frames exactly (100 rounds, the cap); after 40 frames it reaches the top
    frame.  Candidates of the running validators go in the same call: steps of
    different frames in one launch."""
    d = bc.silent_dag(150)
    full = bc.Ref(d)
    full.advance(len(d))
    assert int(full.frames.max()) >= 111
    n40 = int(np.argmax(full.frames >= 40)) + 1            # the first event of frame 40 is in
    ref, lch = bc.Ref(d), gpu_handle(d)
    try:
        done = 0
        for upto, want, rounds in ((n40, 40, 40), (len(d), 101, 100)):
            ref.advance(upto)
            assert np.array_equal(feed(lch, d, done, upto), ref.frames[done:upto])
            done = upto
            _, last_of = ref.tips()
            silent = bc.Cand(0, 2, [0] + [last_of[v] for v in (1, 2, 3)])
            cands = [silent] + ref.tip_candidates([0, 3], only={1, 2, 3})
            exp_f, _ = three_way(lch, ref, cands)
            assert ref.self_parent_frame(silent) == 1 and int(exp_f[0]) == want
            if upto == n40:
                assert want == int(ref.frames[:upto].max())
            f, _ = ask(lch, cands)
            st = lch.build_stats()
            # one wait per round; the cap stops the loop without a last question
            assert st["rounds"] == rounds and st["frame_steps"] > st["rounds"]
            assert len({int(x) for x in f}) >= 2
    finally:
        lch.close()


def test_candidates_without_a_self_parent():
    """seq = 1 for validators without events, with and without other parents:
    frame 1, a root, and nothing is launched."""
    d = shape_dag((16, 40, 5, 0, 0, 1))
    ref, lch = bc.Ref(d), gpu_handle(d)
    try:
        ref.advance(2)
        feed(lch, d, 0, 2)
        cands = [bc.Cand(5, 1, []), bc.Cand(5, 1, [0, 1]), bc.Cand(15, 1, [1])]
        exp_f, exp_r = three_way(lch, ref, cands)
        assert list(exp_f) == [1, 1, 1] and list(exp_r) == [1, 1, 1]
        ask(lch, cands)
        assert lch.build_stats()["launches"] == 0
        # mixed with a candidate that has a self-parent
        mixed = [cands[1]] + ref.tip_candidates([1])
        three_way(lch, ref, mixed)
    finally:
        lch.close()


@pytest.mark.parametrize("V", [63, 65, 257, 1030])
def test_width_edges_fork_free(V):
    """Three events per validator; the quorum sits in the first, a middle and
    the last column (tests/build_cases.py star_dag)."""
    d = bc.star_dag(V)
    ref, lch = bc.Ref(d, light=V > 300), gpu_handle(d)
    try:
        ref.advance(len(d))
        assert np.array_equal(feed(lch, d, 0, len(d), chunk=1024), ref.frames)
        only = {c for c in (0, 1, 31, 32, 62, 63, 64, 65, 255, 256, 1023, 1024, V // 2, V - 2, V - 1) if c < V}
        cands = ref.tip_candidates([0, 3], only=only)
        exp_f, exp_r = three_way(lch, ref, cands)
        assert len(set(map(int, exp_f))) >= 2 and 0 < int(exp_r.sum()) < len(cands)
        # every validator's candidate in one call (n = V) against one call each for a sample
        allc = ref.tip_candidates([3])
        f, r = ask(lch, allc)
        for i in sorted({0, 1, 63, 64, 65, 256, 257, V // 2, V - 1} & set(range(len(allc)))):
            f1, r1 = ask(lch, [allc[i]])
            assert (int(f[i]), int(r[i])) == (int(f1[0]), int(r1[0])), i
    finally:
        lch.close()


def test_width_edge_with_forks():
    """B = 67 branches: the cheater pass and the fork kernel three columns past a wave."""
    d = shape_dag(FORK_EDGE)
    ref, lch = bc.Ref(d), gpu_handle(d)
    try:
        ref.advance(len(d))
        assert np.array_equal(feed(lch, d, 0, len(d)), ref.frames)
        assert lch.ix.num_branches() == 67
        three_way(lch, ref, ref.tip_candidates([0, 3, 57]), one_by_one=False)
    finally:
        lch.close()


def test_batch_of_300_equals_single_calls():
    """n = 300 candidates (the tip candidates repeated): more than one
    64-candidate tile, more than 256 rows of the scratch plane."""
    shape = (24, 30, 6, 5, 6, 2)
    d = shape_dag(shape)
    ref, lch = bc.Ref(d), gpu_handle(d)
    try:
        upto = len(d) // 2
        ref.advance(upto)
        feed(lch, d, 0, upto)
        base = ref.tip_candidates(bc.ks_of(shape))
        cands = [base[(7 * i) % len(base)] for i in range(300)]
        f, r = ask(lch, cands)
        assert lch.build_stats()["fc_pairs"] > 0
        single = {}
        for i, c in enumerate(cands):
            k = (7 * i) % len(base)
            if k not in single:
                f1, r1 = ask(lch, [c])
                single[k] = (int(f1[0]), int(r1[0]))
            assert (int(f[i]), int(r[i])) == single[k], i
        exp_f, exp_r = ref.answers(base)
        for k, v in single.items():
            assert v == (int(exp_f[k]), int(exp_r[k])), k
    finally:
        lch.close()


def test_fc16_option_gives_the_same_frames():
    d = shape_dag((16, 40, 5, 0, 0, 1))
    ref = bc.Ref(d)
    ref.advance(len(d))
    cands = ref.tip_candidates([0, 1, 4, 15])
    exp_f, exp_r = ref.answers(cands)
    for fc16 in (1, 0):
        lch = gpu_handle(d, {"fc16": fc16})
        try:
            feed(lch, d, 0, len(d))
            f, r = ask(lch, cands)
            assert np.array_equal(f, exp_f) and np.array_equal(r, exp_r), fc16
            assert lch.build_stats()["fc16"] == fc16
        finally:
            lch.close()


def test_candidate_seq_0x10000_leaves_the_16_bit_kernel():
    """Every stored seq fits 16 bits (max 0xFFFF), the candidates of the fast
    validators carry seq 0x10000: the packed kernel's gate includes the
    candidate's own seq."""
    import seq16_dags as sd
    V = 12
    dag = sd.two_speed(V, 2, sd.L_LAST16, 40, 5)
    d = bc.Dense(sd.SMALL_W[V], dag.creator, dag.seq, dag.poff, dag.par)
    assert int(d.seq.max()) == 0xFFFF
    ref, lch = bc.Ref(d), gpu_handle(d)
    try:
        ref.advance(len(d))
        feed(lch, d, 0, len(d), chunk=len(d), claimed=ref.frames)
        cands = ref.tip_candidates([0, 1, 3, V - 1])
        assert max(c.seq for c in cands) == 0x10000
        fast = [c for c in cands if c.seq == 0x10000]
        slow = [c for c in cands if c.seq <= 0xFFFF]
        assert fast and slow
        exp_f, exp_r = ref.answers(fast)
        f, r = ask(lch, fast)
        assert np.array_equal(f, exp_f) and np.array_equal(r, exp_r)
        assert lch.build_stats()["fc16"] == 0
        exp_f, exp_r = ref.answers(slow)
        f, r = ask(lch, slow)
        assert np.array_equal(f, exp_f) and np.array_equal(r, exp_r)
        assert lch.build_stats()["fc16"] == 1
        for c in fast[:2] + slow[:2]:
            assert lch.build(c.creator, c.seq, c.parents) == ref.build(c)
    finally:
        lch.close()


def _counting(abft):
    class Counting(abft.DenseLachesis):
        calls = 0

        def _begin(self, *a):
            self.calls += 1
            return super()._begin(*a)

        def _apply(self, *a):
            self.calls += 1
            return super()._apply(*a)

        def _end(self, *a):
            self.calls += 1
            return super()._end(*a)
    return Counting


def _surroundings(lch, mt, anc, sample, n):
    st = lch.state()
    top = int(len(st["root_off"])) - 1
    return dict(
        n_events=lch.ix.num_events(), epoch=st["epoch"], last=st["last_decided_frame"],
        ev_frame=st["ev_frame"].tobytes(), ev_conf=st["ev_confirmed_on"].tobytes(),
        root_off=st["root_off"].tobytes(), root_ev=st["root_ev"].tobytes(),
        top_roots=[lch.frame_roots(f).tobytes() for f in range(max(1, top - 3), top + 2)],
        hb=lch.ix.highest_before_batch(sample), la=lch.ix.lowest_after_batch(sample),
        stats=lch.last_stats(), n_times=mt.num_times(), labels=anc.labels_dense(0, n).tobytes(),
        low=anc.low_water(), calls=lch.calls, blocks=len(lch.blocks))


def test_reads_only():
    """Nothing around the call changes: the index, the abft state, the rows of
    the parents and roots, the last batch's stats, an lx_mt handle with times
    set ahead of Add, an lx_anc handle with labels, no callback.  The contrast:
    one lx_abft_build makes the lx_mt handle forget the times set ahead."""
    import lachesis_hip as lx
    from lachesis_hip import abft
    shape = (24, 30, 6, 5, 6, 2)
    d = shape_dag(shape)
    ref = bc.Ref(d)
    lch = gpu_handle(d, cls=_counting(abft))
    try:
        upto = len(d) // 2
        ref.advance(upto)
        feed(lch, d, 0, upto)
        assert lch.calls > 0

        class _Dagi:
            ix = lch.ix
        mt = lx.mediantime.MedianTimeIndex(_Dagi)
        anc = lx.ancestry.AncestryIndex(_Dagi)
        mt.set_times_dense(0, list(range(1000, 1000 + upto + 50)))      # 50 ahead of Add
        anc.set_labels_dense(0, [1] * (upto // 3))
        cands = ref.tip_candidates(bc.ks_of(shape))
        st = lch.state()
        sample = sorted({p for c in cands for p in c.parents} | set(map(int, st["root_ev"][-40:])))[-64:]
        assert len(sample) == 64
        lch.calls = 0
        before = _surroundings(lch, mt, anc, sample, upto)
        assert before["n_times"] == upto + 50 and before["low"] == upto // 3
        exp_f, exp_r = ref.answers(cands)
        f, r = ask(lch, cands)
        assert np.array_equal(f, exp_f) and np.array_equal(r, exp_r)
        assert lch.build_stats()["launches"] > 0
        for c in cands[:5]:
            ask(lch, [c])
        assert _surroundings(lch, mt, anc, sample, upto) == before
        # existing behaviour, the contrast: lx_abft_build rolls the index back
        assert lch.build(cands[0].creator, cands[0].seq, cands[0].parents) == exp_f[0]
        assert mt.num_times() == upto
        mt.close()
        anc.close()
    finally:
        lch.close()


def test_process_afterwards_is_unchanged():
    """The real events processed after build_frames calls: the same frames,
    blocks and confirmed-on table as a run without the calls."""
    shape = (12, 30, 4, 3, 5, 2)
    d = shape_dag(shape)
    ref = bc.Ref(d)
    plain, asked = gpu_handle(d), gpu_handle(d)
    try:
        done = 0
        for upto in bc.checkpoints(len(d)):
            ref.advance(upto)
            a = feed(plain, d, done, upto, chunk=41)
            b = feed(asked, d, done, upto, chunk=41)
            assert np.array_equal(a, b) and np.array_equal(a, ref.frames[done:upto])
            done = upto
            ask(asked, ref.tip_candidates(bc.ks_of(shape)))
        assert plain.blocks == asked.blocks == ref.abo.blocks and len(plain.blocks) >= 5
        assert np.array_equal(plain.confirmed_on(len(d)), asked.confirmed_on(len(d)))
        for f in range(1, int(ref.frames.max()) + 2):
            assert np.array_equal(plain.frame_roots(f), asked.frame_roots(f))
    finally:
        plain.close()
        asked.close()


def test_errors_before_any_launch():
    from lachesis_hip import abft
    shape = (12, 30, 4, 3, 5, 2)
    d = shape_dag(shape)
    ref = bc.Ref(d)
    lch = gpu_handle(d)
    cold = abft.DenseLachesis(d.weights, bootstrap=False)
    try:
        n = len(d)
        ref.advance(n)
        feed(lch, d, 0, n)
        good = ref.tip_candidates([2])
        by_branch, last_of = ref.tips()
        tips = set(by_branch.values())
        t = good[1].parents[0]
        c, s = good[1].creator, good[1].seq
        off_tip = next(i for i in range(n) if i not in tips)
        other = next(p for p in good[1].parents[1:])
        bad = {
            "creator": bc.Cand(12, 1, []),
            "seq 0": bc.Cand(c, 0, [t]),
            "parent": bc.Cand(c, s, [t, n]),
            "duplicate": bc.Cand(c, s, [t, other, other]),
            "no self-parent": bc.Cand(c, s, [other]),
            "self-parent at another seq": bc.Cand(c, s + 1, [t]),
            "seq 1 with a self-parent": bc.Cand(c, 1, [t]),
            "off the tip": bc.Cand(int(d.creator[off_tip]), int(d.seq[off_tip]) + 1, [off_tip]),
            "seq 1, creator has events": bc.Cand(c, 1, [other]),
        }
        ask(lch, good)
        assert lch.build_stats()["launches"] > 0
        stats = lch.last_stats()
        for name, cand in bad.items():
            for at in (0, 1, len(good)):
                cands = good[:at] + [cand] + good[at:]
                rc, err, _, _ = lch.build_frames(*bc.dense(cands))
                assert (rc, err) == (ERR_ARG, at), (name, at)
                assert lch.build_stats() == dict(launches=0, frame_steps=0, rounds=0, fc16=0, fc_pairs=0), name
        assert lch.last_stats() == stats
        # the refused branch-opening candidates are what lx_abft_build is for
        for name in ("off the tip", "seq 1, creator has events"):
            cand = bad[name]
            assert lch.build(cand.creator, cand.seq, cand.parents) == ref.build(cand), name
        rc, err, f, r = lch.build_frames(*bc.dense([]))
        assert rc == 0 and len(f) == 0 and lch.build_stats()["launches"] == 0
        rc, err, _, _ = cold.build_frames(*bc.dense(good))
        assert rc == ERR_STATE
        # a cheater's fork branch tip may be extended
        forked = [x for x in good if by_branch.get(x.creator) != x.parents[0]]
        assert forked
        exp_f, _ = ref.answers(forked)
        assert np.array_equal(ask(lch, forked)[0], exp_f)
    finally:
        lch.close()
        cold.close()


def test_python_mirror_sets_frames():
    """IndexedLachesis.build_frames(events): e.frame and the is-root flags."""
    import build_model as bm
    ep = bm.Epoch.of_shape((12, 30, 4, 3, 5, 2))
    ep.advance(len(ep.events) // 2)
    from abft_harness import FakeLachesis
    t = FakeLachesis(dict(zip(ep.validators.ids, ep.validators.weights)), backend="gpu")
    consumed, err = t.process_batch(ep.events[:ep.done], claimed=False)
    assert err is None and consumed == ep.done
    cands = ep.tip_candidates([0, 3, 11])
    exp = [ep.oracle_frame(c) for c in cands]
    roots = t.lch.build_frames([c.event for c in cands])
    assert [c.event.frame for c in cands] == exp
    assert roots == [f != ep.self_parent_frame(c) for f, c in zip(exp, cands)]
    assert t.lch.build_stats()["rounds"] >= 1
