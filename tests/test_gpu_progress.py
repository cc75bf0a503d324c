"""lx_abft_build_progress / lx_abft_event_progress: the stake behind each root
of a frame and what the frame's slots add up to (k_root_progress behind the
root-FC kernels), against the CPU model of tests/progress_model.py over the C
oracle's rows.  Every candidate or event a test forms is compared.

Edges the shapes cross: the 32-column LDS chunks and column splits of the
root-FC kernels (V = 63, 65, 257, 1030; B = 67 with forks), the bit-row words
at 32 / 64 roots, more than one 64-candidate tile and more than 256 candidates
(n = 300), sums with bit 30 set under the early-false flag in bit 31, weights
>= 2^16 in the packed kernel, the packed kernel's gate at seq 0x10000, steps
of different frames in one merged launch, the single-step launch (n = 1)."""

import functools

import numpy as np
import pytest

import build_cases as bc
import progress_model as pm

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -1, -4
FRAME_BUILD = 0xFFFFFFFF
SHAPES = [(1, 6, 1, 0, 0, 1), (3, 12, 3, 0, 0, 2), (16, 40, 5, 0, 0, 1), (12, 30, 4, 3, 5, 2), (24, 30, 6, 5, 6, 2)]
WEIGHTED = ((3, 12, 3, 0, 0, 2), (5, 2, 2))
FORK_EDGE = (58, 6, 4, 5, 3, 3)                              # B = 67: three columns past a wave
FIELDS = ("n_roots", "n_caused", "stake", "root_stake")


def gpu_handle(d, options=None, cls=None):
    from lachesis_hip import abft
    lch = (cls or abft.DenseLachesis)(d.weights, event_capacity=len(d) + 8)
    for k, v in (options or {}).items():
        lch.set_option(k, v)
    return lch


def feed(lch, d, lo, hi, chunk=97, claimed=None):
    out = []
    for a in range(lo, hi, chunk):
        b = min(hi, a + chunk)
        c, s, off, par = d.slice(a, b)
        rc, consumed, fr = lch.process_batch(c, s, off, par, None if claimed is None else claimed[a:b])
        assert rc == 0 and consumed == b - a
        out.append(fr)
    return np.concatenate(out) if out else np.zeros(0, dtype=np.uint32)


@functools.lru_cache(maxsize=None)
def shape_dag(shape, weights=None):
    return bc.shape_dag(shape, weights)


def roots_of(ref):
    """{frame: root events in slot order} of the oracle."""
    if ref.light:
        return {f: list(r) for f, r in ref.roots.items()}
    out, f = {}, 1
    while len(ref.abo.frame_roots(f)):
        out[f] = [int(r) for r in ref.abo.frame_roots(f)]
        f += 1
    return out


def model_of(ref, lch):
    m = pm.ProgressModel.from_ref(ref, roots_of(ref))
    for f, rs in m.roots.items():                            # the engine's slots, in its order
        assert list(lch.frame_roots(f)) == rs
    assert len(lch.frame_roots(max(m.roots, default=0) + 1)) == 0
    return m


def same(got, i, exp, what):
    for k in FIELDS:
        assert int(got[k][i]) == exp[k], (what, k, int(got[k][i]), exp[k])


def same_pairs(lch, n, exps, what):
    off, root, stake, total = lch.progress_pairs(n)
    assert int(off[0]) == 0 and int(off[n]) == total == len(root) == sum(len(e["pairs"]) for e in exps)
    for i, e in enumerate(exps):
        a, b = int(off[i]), int(off[i + 1])
        assert list(zip(map(int, root[a:b]), map(int, stake[a:b]))) == e["pairs"], (what, i)


def ask(lch, cands, at=None, pairs=True):
    rc, err, got = lch.build_progress(*bc.dense(cands), at_frame=at, pairs=pairs)
    assert rc == 0, lch.L.lx_abft_last_error(lch.h).decode()
    return got


def check_candidates(lch, m, cands, one_by_one=True, what=""):
    """One call with pairs (and one per candidate) against the model; the
    frames against lx_abft_build_frames.  Returns the model's answers."""
    exps = []
    for c in cands:
        spf, F = m.build_frame(c)
        e = m.progress(c, F)
        e["frame"], e["spf"] = F, spf
        exps.append(e)
    got = ask(lch, cands)
    for i, e in enumerate(exps):
        assert int(got["frame"][i]) == e["frame"], (what, i)
        same(got, i, e, (what, i))
    same_pairs(lch, len(cands), exps, what)
    rc, err, frames, _ = lch.build_frames(*bc.dense(cands))
    assert rc == 0 and np.array_equal(frames, got["frame"])
    if one_by_one:
        for i, c in enumerate(cands):
            g1 = ask(lch, [c])
            assert int(g1["frame"][0]) == exps[i]["frame"]
            same(g1, 0, exps[i], (what, i, "alone"))
            same_pairs(lch, 1, [exps[i]], (what, i, "alone"))
    return exps


@pytest.mark.parametrize("shape,weights", [(s, None) for s in SHAPES] + [WEIGHTED],
                         ids=lambda x: "-".join(map(str, x)) if x else "eq")
def test_shapes_at_three_checkpoints(shape, weights):
    d = shape_dag(shape, weights)
    ref, lch = bc.Ref(d), gpu_handle(d)
    try:
        done, partial, caused = 0, 0, 0
        for upto in bc.checkpoints(len(d)):
            ref.advance(upto)
            assert np.array_equal(feed(lch, d, done, upto, chunk=37), ref.frames[done:upto])
            done = upto
            m = model_of(ref, lch)
            cands = ref.tip_candidates(bc.ks_of(shape))
            for e, c in zip(check_candidates(lch, m, cands, what=upto), cands):
                assert e["frame"] == ref.build(c)
                assert e["stake"] < m.quorum
                partial += sum(0 < s < m.quorum for _, s in e["pairs"])
                caused += e["n_caused"]
        if shape[0] > 1:
            assert partial >= 10 and caused >= 10
        else:
            assert partial == caused == 0
    finally:
        lch.close()


@pytest.mark.parametrize("shape", [(16, 40, 5, 0, 0, 1), (24, 30, 6, 5, 6, 2)], ids=lambda x: "-".join(map(str, x)))
def test_explicit_frames(shape):
    """Each frame of every candidate's climb asked alone, all in one call
    together with Build entries: steps of different frames in one launch."""
    d = shape_dag(shape)
    ref, lch = bc.Ref(d), gpu_handle(d)
    try:
        ref.advance(len(d))
        feed(lch, d, 0, len(d))
        m = model_of(ref, lch)
        top = max(m.roots)
        cands, at, exps, below = [], [], [], []
        for c in ref.tip_candidates(bc.ks_of(shape)):
            spf, F = m.build_frame(c)
            row = m.virtual_row(c)
            for f in list(range(max(spf, 1), F + 1)) + [FRAME_BUILD, top + 1, top + 7]:
                g = F if f == FRAME_BUILD else f
                e = m.progress(c, g, row)
                e["frame"] = g
                cands.append(c)
                at.append(f)
                exps.append(e)
                below.append(g < F)
        assert sum(below) >= 10 and len({e["frame"] for e in exps}) >= 4
        got = ask(lch, cands, at=at)
        for i, e in enumerate(exps):
            assert int(got["frame"][i]) == e["frame"]
            same(got, i, e, i)
            if at[i] in (top + 1, top + 7):
                assert [int(got[k][i]) for k in FIELDS] == [0, 0, 0, 0]
            elif e["frame"] <= top:
                assert (int(got["stake"][i]) >= m.quorum) == below[i], i
        same_pairs(lch, len(cands), exps, "explicit")
        # the same entries alone: the single-step launch, no frame loop behind an explicit entry
        for i in range(len(cands)):
            g1 = ask(lch, [cands[i]], at=[at[i]])
            same(g1, 0, exps[i], (i, "alone"))
            same_pairs(lch, 1, [exps[i]], (i, "alone"))
            if at[i] != FRAME_BUILD:
                assert lch.build_stats()["rounds"] == (1 if at[i] <= top else 0)
    finally:
        lch.close()


def test_candidates_without_a_self_parent():
    """Validator 3 of 4 has no events: its first event gets frame 1 without
    roots(1) being asked; its progress over roots(1) is reported as it is and
    reaches the quorum when it sees the three others."""
    creator, seq, poff, par, last = [], [], [0], [], [-1, -1, -1]
    for k in range(4):
        for c in range(3):
            ps = ([last[c]] if last[c] >= 0 else []) + [last[o] for o in range(3) if o != c and last[o] >= 0]
            creator.append(c)
            seq.append(k + 1)
            par.extend(ps)
            poff.append(len(par))
            last[c] = len(creator) - 1
    d = bc.Dense([1, 1, 1, 1], creator, seq, poff, par)
    ref, lch = bc.Ref(d), gpu_handle(d)
    try:
        ref.advance(len(d))
        feed(lch, d, 0, len(d))
        m = model_of(ref, lch)
        cands = [bc.Cand(3, 1, []), bc.Cand(3, 1, last), bc.Cand(3, 1, [0]), bc.Cand(3, 1, [last[1], 2])]
        exps = check_candidates(lch, m, cands)
        assert [e["frame"] for e in exps] == [1, 1, 1, 1]
        assert exps[0]["stake"] == 0 and exps[0]["n_roots"] == len(m.roots[1]) > 0
        assert exps[1]["stake"] >= m.quorum and exps[1]["n_caused"] == exps[1]["n_roots"]
        assert 0 < exps[2]["root_stake"] < m.quorum
        # mixed with candidates that have a self-parent, and at explicit frames
        mixed = [cands[1]] + ref.tip_candidates([0, 2]) + [cands[3]]
        check_candidates(lch, m, mixed, one_by_one=False)
        got = ask(lch, [cands[1], cands[1]], at=[2, 1])
        same(got, 0, m.progress(cands[1], 2), "frame 2")
        same(got, 1, exps[1], "frame 1")
    finally:
        lch.close()


@pytest.mark.parametrize("V", [63, 65, 257, 1030])
def test_width_edges_fork_free(V):
    d = bc.star_dag(V)
    ref, lch = bc.Ref(d, light=V > 300), gpu_handle(d)
    try:
        ref.advance(len(d))
        assert np.array_equal(feed(lch, d, 0, len(d), chunk=1024), ref.frames)
        m = model_of(ref, lch)
        assert max(len(r) for r in m.roots.values()) >= V    # bit rows past 32 and 64 roots
        # the model's R x B planes per candidate and frame cost seconds at V = 1030: fewer creators there
        only = {c for c in ((0, 1, 63, 64, 1023, 1024, V // 2, V - 1) if V > 300 else
                            (0, 1, 31, 32, 62, 63, 64, 65, 255, 256, V // 2, V - 2, V - 1)) if c < V}
        cands = ref.tip_candidates([0, 3], only=only)
        exps = check_candidates(lch, m, cands, one_by_one=V < 300)
        assert len({e["frame"] for e in exps}) >= 2
        assert any(0 < e["stake"] < m.quorum for e in exps) and any(e["n_caused"] for e in exps)
        # every frame below the Build frame in one call: quorums are met there
        c2, at2, exp2 = [], [], []
        for c, e in zip(cands, exps):
            for f in range(1, e["frame"]):
                c2.append(c)
                at2.append(f)
                exp2.append(m.progress(c, f))
        assert sum(e["stake"] >= m.quorum and e["n_caused"] >= 3 for e in exp2) >= len(cands)
        got = ask(lch, c2, at=at2)
        for i, e in enumerate(exp2):
            same(got, i, e, (i, at2[i]))
        same_pairs(lch, len(c2), exp2, "below")
    finally:
        lch.close()


def test_width_edge_with_forks():
    d = shape_dag(FORK_EDGE)
    ref, lch = bc.Ref(d), gpu_handle(d)
    try:
        ref.advance(len(d))
        assert np.array_equal(feed(lch, d, 0, len(d)), ref.frames)
        assert lch.ix.num_branches() == 67
        m = model_of(ref, lch)
        exps = check_candidates(lch, m, ref.tip_candidates([0, 3, 57]), one_by_one=False)
        assert any(s == 0 for e in exps for _, s in e["pairs"]) and any(e["n_caused"] for e in exps)
    finally:
        lch.close()


def test_batch_of_300():
    """n = 300 candidates (the tip candidates repeated): more than one
    64-candidate tile, more than 256 rows of the scratch plane."""
    shape = (24, 30, 6, 5, 6, 2)
    d = shape_dag(shape)
    ref, lch = bc.Ref(d), gpu_handle(d)
    try:
        upto = len(d) // 2
        ref.advance(upto)
        feed(lch, d, 0, upto)
        m = model_of(ref, lch)
        base = ref.tip_candidates(bc.ks_of(shape))
        exp_base = check_candidates(lch, m, base, one_by_one=False)
        idx = [(7 * i) % len(base) for i in range(300)]
        got = ask(lch, [base[k] for k in idx])
        for i, k in enumerate(idx):
            assert int(got["frame"][i]) == exp_base[k]["frame"]
            same(got, i, exp_base[k], i)
        same_pairs(lch, 300, [exp_base[k] for k in idx], "300")
    finally:
        lch.close()


BIG = 1 << 27


@pytest.mark.parametrize("shape,weights", [((16, 40, 5, 0, 0, 1), (BIG,) * 15 + (BIG - 1,)),
                                           ((12, 30, 4, 3, 5, 2), (BIG,) * 11 + ((1 << 31) - 1 - 11 * BIG,))],
                         ids=["fork-free", "forks"])
def test_stakes_summing_to_2_31_minus_1(shape, weights):
    """Sums have bit 30 set; bit 31 stays the early-false flag.  Every weight
    is >= 2^16: the high halves of the packed kernel.  fc16 = 0 and 1 agree."""
    assert sum(weights) == (1 << 31) - 1
    d = shape_dag(shape, weights)
    ref = bc.Ref(d)
    ref.advance(len(d))
    cands = ref.tip_candidates(bc.ks_of(shape))
    outs = []
    for fc16 in (1, 0):
        lch = gpu_handle(d, {"fc16": fc16})
        try:
            feed(lch, d, 0, len(d))
            m = model_of(ref, lch)
            exps = check_candidates(lch, m, cands, one_by_one=False)
            assert lch.build_stats()["fc16"] == (fc16 if not shape[3] else 0)
            assert any(s >> 30 for e in exps for _, s in e["pairs"])
            if shape[3]:
                assert any(s == 0 for e in exps for _, s in e["pairs"])
            outs.append(exps)
        finally:
            lch.close()
    assert outs[0] == outs[1]


def test_candidate_seq_0x10000_leaves_the_16_bit_kernel():
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
        fast = [c for c in cands if c.seq == 0x10000]
        slow = [c for c in cands if c.seq <= 0xFFFF]
        assert fast and slow
        lo, top = min(ref.self_parent_frame(c) for c in cands), int(ref.frames.max())
        roots = {f: [int(r) for r in lch.frame_roots(f)] for f in range(max(1, lo), top + 1)}
        m = pm.ProgressModel.from_ref(ref, roots)            # the frames the candidates can reach
        check_candidates(lch, m, fast, one_by_one=False)
        assert lch.build_stats()["fc16"] == 0
        check_candidates(lch, m, slow, one_by_one=False)
        rc, err, got = lch.build_progress(*bc.dense(slow))
        assert rc == 0 and lch.build_stats()["fc16"] == 1
    finally:
        lch.close()


@pytest.mark.parametrize("shape,weights", [(s, None) for s in SHAPES] + [WEIGHTED],
                         ids=lambda x: "-".join(map(str, x)) if x else "eq")
def test_indexed_events(shape, weights):
    d = shape_dag(shape, weights)
    ref, lch = bc.Ref(d), gpu_handle(d)
    try:
        n = len(d)
        ref.advance(n)
        assert np.array_equal(feed(lch, d, 0, n), ref.frames)
        m = model_of(ref, lch)
        evs = list(range(n))
        rc, err, got = lch.event_progress(evs, pairs=True)
        assert rc == 0 and np.array_equal(got["frame"], ref.frames)
        exps = [m.event_progress(e, int(ref.frames[e])) for e in evs]
        own = 0
        for e in evs:
            same(got, e, exps[e], e)
            # by construction of calcFrameIdx -- except for an event without a
            # self-parent (a cheater's second first event sees the others'):
            # frame 1 is given without roots(1) being asked
            assert int(got["stake"][e]) < m.quorum or d.seq[e] == 1, e
            if e in m.roots.get(int(ref.frames[e]), []):
                own += 1
                assert exps[e]["n_caused"] == sum(s >= m.quorum for r, s in exps[e]["pairs"] if r != e)
        assert own >= min(n, 6)
        same_pairs(lch, n, exps, "own frame")
        off, root, stake, total = lch.progress_pairs(n)
        a = np.repeat(np.array(evs, dtype=np.uint32), np.diff(off).astype(np.int64))
        assert np.array_equal(stake >= m.quorum, lch.ix.forkless_cause_batch(a, root).astype(bool))
        # every earlier frame back to the self-parent's frame
        ev2, at2 = [], []
        for e in evs:
            spf = m.self_parent_frame(bc.Cand(d.creator[e], d.seq[e], d.parents(e)))
            for g in range(max(spf, 1), int(ref.frames[e])):
                ev2.append(e)
                at2.append(g)
        if shape[0] > 1:
            assert len(ev2) >= 10
        if ev2:
            rc, err, got2 = lch.event_progress(ev2, at_frame=at2, pairs=True)
            assert rc == 0 and list(got2["frame"]) == at2
            exps2 = [m.event_progress(e, g) for e, g in zip(ev2, at2)]
            for i, x in enumerate(exps2):
                same(got2, i, x, (ev2[i], at2[i]))
                assert int(got2["stake"][i]) >= m.quorum
            same_pairs(lch, len(ev2), exps2, "earlier frames")
        rc, err, g1 = lch.event_progress([n - 1])           # one event: the single-step launch
        assert rc == 0
        same(g1, 0, exps[n - 1], "alone")
    finally:
        lch.close()


def test_reads_only():
    """The surroundings test_gpu_build_frames.py::test_reads_only snapshots,
    taken around both calls; the rest of the epoch processed afterwards gives
    the frames and block log of a handle that never asked."""
    import lachesis_hip as lx
    from lachesis_hip import abft
    import test_gpu_build_frames as tb
    shape = (24, 30, 6, 5, 6, 2)
    d = shape_dag(shape)
    ref = bc.Ref(d)
    lch = gpu_handle(d, cls=tb._counting(abft))
    plain = gpu_handle(d)
    try:
        upto = len(d) // 2
        ref.advance(upto)
        feed(lch, d, 0, upto)
        feed(plain, d, 0, upto)

        class _Dagi:
            ix = lch.ix
        mt = lx.mediantime.MedianTimeIndex(_Dagi)
        anc = lx.ancestry.AncestryIndex(_Dagi)
        mt.set_times_dense(0, list(range(1000, 1000 + upto + 50)))      # 50 ahead of Add
        anc.set_labels_dense(0, [1] * (upto // 3))
        cands = ref.tip_candidates(bc.ks_of(shape))
        st = lch.state()
        sample = sorted({p for c in cands for p in c.parents} | set(map(int, st["root_ev"][-40:])))[-64:]
        lch.calls = 0
        before = tb._surroundings(lch, mt, anc, sample, upto)
        assert before["n_times"] == upto + 50 and before["low"] == upto // 3
        m = model_of(ref, lch)
        check_candidates(lch, m, cands, one_by_one=False)
        assert lch.build_stats()["launches"] > 0
        top = max(m.roots)
        ask(lch, cands[:7], at=[top, 1, FRAME_BUILD, top + 1, 2, top - 1, 1], pairs=False)
        rc, err, got = lch.event_progress(list(range(upto)), pairs=True)
        assert rc == 0 and lch.build_stats()["launches"] > 0
        rc, err, got = lch.event_progress([upto - 1, 0], at_frame=[1, top])
        assert rc == 0
        assert tb._surroundings(lch, mt, anc, sample, upto) == before
        mt.close()
        anc.close()
        ref.advance(len(d))
        a, b = feed(lch, d, upto, len(d), chunk=41), feed(plain, d, upto, len(d), chunk=41)
        assert np.array_equal(a, b) and np.array_equal(a, ref.frames[upto:])
        assert lch.blocks == plain.blocks == ref.abo.blocks and len(plain.blocks) >= 5
        assert np.array_equal(plain.confirmed_on(len(d)), lch.confirmed_on(len(d)))
    finally:
        lch.close()
        plain.close()


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
        zero = dict(launches=0, frame_steps=0, rounds=0, fc16=0, fc_pairs=0)
        ask(lch, good)
        assert lch.build_stats()["launches"] > 0
        stats = lch.last_stats()
        for name, cand in bad.items():
            for at in (0, 1, len(good)):
                cands = good[:at] + [cand] + good[at:]
                rc, err, _ = lch.build_progress(*bc.dense(cands), pairs=True)
                assert (rc, err) == (ERR_ARG, at), (name, at)
                assert lch.build_stats() == zero, name
                assert lch.progress_pairs(0)[3] == 0
        for at in (0, 2, len(good) - 1):                     # at_frame 0
            frames = [FRAME_BUILD] * len(good)
            frames[at] = 0
            rc, err, _ = lch.build_progress(*bc.dense(good), at_frame=frames)
            assert (rc, err) == (ERR_ARG, at) and lch.build_stats() == zero
            rc, err, _ = lch.event_progress(list(range(len(good))), at_frame=frames)
            assert (rc, err) == (ERR_ARG, at) and lch.build_stats() == zero
        for at in (0, 3):                                    # an event out of range
            evs = [0, 1, 2, 3, 4]
            evs[at] = n
            rc, err, _ = lch.event_progress(evs)
            assert (rc, err) == (ERR_ARG, at) and lch.build_stats() == zero
        for flags in (2, 3, 0x80000000):                     # unknown flag bits
            rc, err, _ = lch.build_progress(*bc.dense(good), flags=flags)
            assert (rc, err) == (ERR_ARG, 0) and lch.build_stats() == zero
            rc, err, _ = lch.event_progress([0, 1], flags=flags)
            assert (rc, err) == (ERR_ARG, 0) and lch.build_stats() == zero
        assert lch.last_stats() == stats
        rc, err, got = lch.build_progress(*bc.dense([]))
        assert rc == 0 and len(got["frame"]) == 0 and lch.build_stats() == zero
        rc, err, got = lch.event_progress([])
        assert rc == 0 and len(got["frame"]) == 0 and lch.build_stats() == zero
        rc, err, _ = cold.build_progress(*bc.dense(good))
        assert rc == ERR_STATE
        rc, err, _ = cold.event_progress([0])
        assert rc == ERR_STATE
        # a cheater's fork branch tip may be extended
        forked = [x for x in good if by_branch.get(x.creator) != x.parents[0]]
        assert forked
        check_candidates(lch, model_of(ref, lch), forked, one_by_one=False)
    finally:
        lch.close()
        cold.close()


def test_pair_reader():
    shape = (16, 40, 5, 0, 0, 1)
    d = shape_dag(shape)
    ref, lch = bc.Ref(d), gpu_handle(d)
    try:
        upto = len(d) // 2
        ref.advance(upto)
        feed(lch, d, 0, upto)
        m = model_of(ref, lch)
        cands = ref.tip_candidates([0, 4])
        exps = check_candidates(lch, m, cands, one_by_one=False)
        ask(lch, cands)
        flat = [p for e in exps for p in e["pairs"]]
        n = len(cands)
        assert len(flat) > 40
        for cap in (0, 1, len(exps[0]["pairs"]) + 3, len(flat) - 1, len(flat), len(flat) + 5):
            off, root, stake, total = lch.progress_pairs(n, cap=cap)
            k = min(cap, len(flat))
            assert total == len(flat) and len(root) == k
            assert list(zip(map(int, root), map(int, stake))) == flat[:k]
            assert list(map(int, off)) == list(np.cumsum([0] + [len(e["pairs"]) for e in exps]))
        # empty after a call without the flag, after build_frames, after a batch
        ask(lch, cands, pairs=False)
        assert lch.progress_pairs(0)[3] == 0
        ask(lch, cands)
        assert lch.progress_pairs(n)[3] == len(flat)
        assert lch.build_frames(*bc.dense(cands))[0] == 0
        assert lch.progress_pairs(0)[3] == 0
        ask(lch, cands)
        rc, err, got = lch.event_progress([0, 1])
        assert rc == 0 and lch.progress_pairs(0)[3] == 0
        ask(lch, cands)
        feed(lch, d, upto, upto + 5)
        assert lch.progress_pairs(0)[3] == 0
    finally:
        lch.close()


def test_python_mirror():
    """IndexedLachesis.build_progress / event_progress / progress_pairs."""
    import build_model as bm
    ep = bm.Epoch.of_shape((12, 30, 4, 3, 5, 2))
    ep.advance(len(ep.events) // 2)
    from abft_harness import FakeLachesis
    t = FakeLachesis(dict(zip(ep.validators.ids, ep.validators.weights)), backend="gpu")
    consumed, err = t.process_batch(ep.events[:ep.done], claimed=False)
    assert err is None and consumed == ep.done
    m = pm.ProgressModel(ep)
    cands = ep.tip_candidates([0, 3, 11])
    got = t.lch.build_progress([c.event for c in cands], pairs=True)
    off, root_ids, stake, total = t.lch.progress_pairs()
    for i, c in enumerate(cands):
        spf, F = m.frame(c)
        e = m.progress(c, F)
        assert int(got["frame"][i]) == F
        same(got, i, e, i)
        a, b = int(off[i]), int(off[i + 1])
        assert [(ep.pos(r), int(s)) for r, s in zip(root_ids[a:b], stake[a:b])] == e["pairs"]
    evs = ep.events[:ep.done]
    got = t.lch.event_progress(evs)
    for i in range(len(evs)):
        same(got, i, m.event_progress(i, int(m.frames[i])), i)
