"""tests/selection_cases.py on the CPU: the numpy models against the
independent pure-Python ones (median_time_model.median_time,
oracle.emitter_oracle.QuorumIndexer) on every case class, and every generator
reaches the edge it is for."""

import numpy as np
import pytest

import median_time_model as mm
import selection_cases as sc
from median_time_model import FORK, NONE, SEEN
from oracle import emitter_oracle as eo
from oracle import vecfc_oracle as vo

WIDTHS = [1, 3, 7, 65]


# ----------------------------------------------------------------------------
# DAGs and weights

@pytest.mark.parametrize("V,hub", [(1, 0), (2, 0), (3, 0), (7, 0), (12, 0), (13, 5), (65, 37), (100, 0)])
def test_comb_rows_in_closed_form(V, hub):
    d = sc.comb_dag(V, hub=hub, second_layer=True)
    o = sc.oracle_of([1] * V, d.arrays())
    q = sc.QiModel([1] * V, o, d.creator)
    assert o.num_branches() == V
    assert max(d.poff[i + 1] - d.poff[i] for i in range(len(d))) <= 12
    assert len(d) == V + d.K + (V - 1) and d.K == max(1, -(-(V - 1) // 11))
    for ev in range(len(d)):
        assert np.array_equal(q.seqs(ev), sc.comb_row(d, ev)), ev
    assert (sc.comb_row(d, d.chain[-1]) > 0).all()                       # c_K observes everyone
    if V > 24:
        assert len({d.j_of[v] for v in d.others}) == d.K                 # j(v) takes every value
        mid = sc.comb_row(d, d.chain[d.K // 2 - 1])
        assert 0 < (mid > 0).sum() < V                                   # a mid-chain event: a prefix


def test_fork3_dag_sees_both_forks():
    d = sc.fork3_dag()
    o = sc.oracle_of(sc.FORK3_WEIGHTS, d.arrays())
    q = sc.QiModel(sc.FORK3_WEIGHTS, o, d.creator)
    assert o.num_branches() == 5
    assert list(q.seqs(d.narrow)) == [2, 2, 2]
    assert list(q.seqs(d.wide)) == [3, sc.FORK_SEQ, sc.FORK_SEQ]


@pytest.mark.parametrize("V", [2, 3, 7, 63, 65, 1025, 7169])
def test_weight_vectors(V):
    w = sc.mixed_weights(V)
    assert len(w) == V and min(w) == 1 and sum(w) < 1 << 31
    assert max(w) <= w.count(1) or V == 2
    if V >= 8:
        assert len(set(w)) > 2
    h = sc.heavy_weights(V, big=V // 2)
    assert sum(h) == (1 << 31) - 1 and len(h) == V
    dw = sc.dominant_weights(V)
    assert dw[0] == 1 << 30 and dw[0] > sum(dw[1:])
    # every sum up to the total is reachable, from any side
    total = sum(w)
    for target in {0, 1, 2, total // 2 - 1, total // 2, total // 2 + 1, sc.quorum_of(w), total}:
        for where in ("start", "end", "middle"):
            S = sc.subset_with_sum(w, target, sc.placed_order(list(range(V)), where))
            assert sum(w[v] for v in S) == target and len(set(S)) == len(S)
    with pytest.raises(AssertionError):
        sc.subset_with_sum(w, total + 1, range(V))


# ----------------------------------------------------------------------------
# MedianTime

def _mt_model(V):
    d = sc.comb_dag(V)
    return d, sc.MtModel(sc.mixed_weights(V), d.arrays())


def _py_median(q, case):
    """median_time_model.median_time over (kind, time) pairs."""
    row = q.merged_row(case.t)
    entries = [(int(k), int(t)) for k, t in zip(q.kind, row)]
    return mm.median_time(entries, q.m.w, case.default)


def _queries(d, m):
    out = [m.query(d.chain[-1]), m.query(d.V // 2)]
    if d.K > 1:
        out.append(m.query(d.chain[d.K // 2 - 1]))
    return out


@pytest.mark.parametrize("V", WIDTHS)
def test_mt_model_matches_python_on_every_class(V):
    d, m = _mt_model(V)
    n = 0
    for q in _queries(d, m):
        cases = sc.spread_cases(q)
        if q.ev == d.chain[-1] and q.half >= 1:
            cases += sc.ladder_cases(q)
        for case in cases:
            got = q.median(case.t, case.default)
            assert got == _py_median(q, case), (q.ev, case)
            if case.expect is not None:
                assert got == case.expect, (q.ev, case)
            # the event times the GPU test uploads give this row back
            t = q.event_times(case.t)
            assert np.array_equal(t[q.src], np.asarray(case.t, dtype=np.uint64))
            n += 1
    assert n >= 30
    names = {c.name.split("-")[0] for c in sc.spread_cases(m.query(d.chain[-1]))}
    assert names == {"uniform", "window", "equal", "extremes", "all"}


@pytest.mark.parametrize("V", [3, 7, 65])
def test_mt_queries_cover_observed_and_default(V):
    d, m = _mt_model(V)
    top, root = m.query(d.chain[-1]), m.query(V // 2)
    assert len(top.obs) == V and (top.kind == SEEN).all()
    assert list(root.obs) == [V // 2] and (root.kind == NONE).sum() == V - 1
    # the unobserved rest weighs in at the default time
    assert root.median(np.array([9], dtype=np.uint64), 4) == 4
    assert root.median(np.array([9], dtype=np.uint64), 1 << 40) == (9 if m.w[V // 2] >= root.half else 1 << 40)
    if d.K > 1:
        mid = m.query(d.chain[d.K // 2 - 1])
        assert 1 < len(mid.obs) < V


@pytest.mark.parametrize("V", [3, 7, 65])
def test_ladder_reaches_every_bit_at_the_edge(V):
    d, m = _mt_model(V)
    q = m.query(d.chain[-1])
    cases = sc.ladder_cases(q)
    assert len(cases) == 64 * 3
    seen = set()
    for c in cases:
        b, lo, hi = c.info["bit"], c.info["lo"], c.info["hi"]
        assert (lo ^ hi).bit_length() - 1 == b                            # first differ exactly at b
        assert lo < hi and lo >> (b + 1) == hi >> (b + 1)
        low = c.info["low"]
        assert sum(q.m.w[v] for v in low) == c.info["target"] == q.half + c.info["step"]
        vals = set(map(int, c.t))
        assert vals <= {lo, hi} and int((np.asarray(c.t) == np.uint64(lo)).sum()) == len(low)
        got = q.median(c.t, c.default)
        assert got == c.expect == (hi if c.info["step"] < 0 else lo)     # flips between half - 1 and half
        assert got == _py_median(q, c)
        seen.add((b, c.info["step"]))
    assert seen == {(b, s) for b in range(64) for s in sc.LADDER_STEPS}
    if V >= 65:
        # non-trivial prefixes and lower bits occur
        assert any(c.info["hi"] >> (c.info["bit"] + 1) for c in cases if c.info["bit"] < 60)
        assert any(c.info["lo"] & ((1 << c.info["bit"]) - 1) for c in cases if c.info["bit"] > 4)


def test_window_cases_share_a_prefix():
    d, m = _mt_model(65)
    q = m.query(d.chain[-1])
    for c in sc.spread_cases(q):
        if c.name.startswith("window"):
            t = [int(x) for x in c.t]
            x, k = c.info["x"], c.info["k"]
            assert x >> 61 == 0b101 and all(x <= v < x + (1 << k) for v in t)
            assert len(set(t)) > 1
            top = (min(t) ^ max(t)).bit_length() - 1
            assert top <= k + 1 and max(t) >> (top + 1) != 0              # a non-trivial common prefix
        if c.name.startswith("extremes"):
            t = set(map(int, c.t))
            assert 0 in t and sc.MASK64 in t
    assert {c.default for c in sc.spread_cases(q) if c.name.startswith("extremes")} == set(sc.DEFAULT_TIMES)


@pytest.mark.parametrize("V", [7, 65])
def test_dominant_validator_decides(V):
    d = sc.comb_dag(V)
    m = sc.MtModel(sc.dominant_weights(V), d.arrays())
    q = m.query(d.chain[-1])
    cases = sc.dominant_cases(q)
    assert [c.name for c in cases] == ["dominant-smallest", "dominant-largest", "dominant-middle"]
    for c in cases:
        t = [int(x) for x in c.t]
        rank = sum(1 for x in t[1:] if x < t[0])
        assert {"dominant-smallest": rank == 0, "dominant-largest": rank == V - 1,
                "dominant-middle": 0 < rank < V - 1}[c.name]
        assert q.median(c.t, c.default) == c.expect == t[0] == _py_median(q, c)


def test_half_zero_cases():
    # V = 1, weight 1
    d = sc.comb_dag(1)
    m = sc.MtModel([1], d.arrays())
    for ev in range(len(d)):
        q = m.query(ev)
        assert q.honest == 1 and q.half == 0
        for c in sc.spread_cases(q):
            assert q.median(c.t, c.default) == int(c.t[0]) == _py_median(q, c)
    # honest weight 1 beside two cheaters: the cheaters' zero
    f = sc.fork3_dag()
    m = sc.MtModel(sc.FORK3_WEIGHTS, f.arrays())
    q = m.query(f.wide)
    assert list(q.kind) == [SEEN, FORK, FORK] and q.honest <= 1 and q.half == 0
    for c in sc.spread_cases(q):
        assert q.median(c.t, c.default) == 0 == _py_median(q, c)
    q = m.query(f.narrow)
    assert (q.kind == SEEN).all() and q.half == 5
    for c in sc.spread_cases(q):
        assert q.median(c.t, c.default) == _py_median(q, c)


# ----------------------------------------------------------------------------
# QuorumIndexer

class _Merged:
    """dagi of the pure-Python QuorumIndexer over the C oracle's rows."""

    def __init__(self, o):
        self.o = o

    def get_merged_highest_before(self, ev):
        return vo.HighestBeforeSeq(raw=self.o.merged_hb(ev))


class _Vals:
    """What eo.QuorumIndexer needs of a validator set, idx order as given."""

    def __init__(self, w):
        self.weights = list(w)
        self.idxs = {v: v for v in range(len(w))}

    def __len__(self):
        return len(self.weights)

    def quorum(self):
        return sc.quorum_of(self.weights)


class _Ev:
    def __init__(self, ev, creator):
        self.id, self.creator = ev, creator


def _qi_pair(d, w, cap):
    o = sc.oracle_of(w, d.arrays())
    q = sc.QiModel(w, o, d.creator)
    p = eo.QuorumIndexer(_Vals(w), _Merged(o), eo.capped_metric(list(w), cap))
    return q, p


def _process_both(d, q, p, evs, flags):
    q.process(evs, flags)
    for ev, f in zip(evs, flags):
        p.process_event(_Ev(ev, d.creator[ev]), bool(f))


def _same_state(q, p):
    assert np.array_equal(q.matrix(), np.array(p.get_global_matrix()))
    assert list(q.sp) == p.get_self_parent_seqs()
    assert list(q.medians()) == p.get_global_median_seqs()


@pytest.mark.parametrize("V", WIDTHS)
def test_quorum_edge_cases_sit_on_the_quorum(V):
    d = sc.comb_dag(V, hub=sc.qi_hub(V), second_layer=True)
    w = sc.mixed_weights(V)
    Q = sc.quorum_of(w)
    cases = sc.quorum_edge_cases(d, w)
    assert {(name[:-2], int(name[-2:])) for name, *_ in cases} >= {(p, s) for p in ("start", "end", "middle")
                                                                    for s in (-1, 0)}
    assert len(cases) == (9 if V > 1 else 6)
    sets = {}
    for name, evs, u, S, target in cases:
        assert sum(w[c] for c in S) == target == Q + int(name[-2:])      # exactly Q - 1, Q, Q + 1
        assert sorted(d.creator[e] for e in evs) == sorted(S)
        q, p = _qi_pair(d, w, 2)
        _process_both(d, q, p, evs, [0] * len(evs))
        assert all(q.seqs(e)[u] >= 1 for e in evs)                        # every one observes root u
        assert not q.matrix()[:, [c for c in range(V) if c not in S]].any()
        _same_state(q, p)
        med = int(q.medians()[u])
        assert (med == 0) if target < Q else (med >= 1), name
        sets[name] = tuple(S)
    if V >= 65:
        assert len({sets["start+0"], sets["end+0"], sets["middle+0"]}) == 3
        assert min(sets["end+0"]) > min(sets["start+0"]) and max(sets["start+0"]) < max(sets["end+0"])


@pytest.mark.parametrize("V", WIDTHS)
def test_whole_matrix_plan_matches_python(V):
    d = sc.comb_dag(V, hub=sc.qi_hub(V), second_layer=True)
    w = sc.mixed_weights(V)
    me = d.hub
    evs, flags = sc.whole_matrix_plan(d, me)
    assert set(d.layer2.values()) <= set(evs) and set(d.chain) <= set(evs)
    assert sum(flags) == len([e for e in evs if d.creator[e] == me]) >= 1
    if V >= 65:
        # a creator's later event wins, and it is not its newest
        last = {}
        for e in evs:
            last[d.creator[e]] = e
        assert last[d.hub] != d.chain[-1] and evs.count(last[d.hub]) == 2
        assert any(last[v] == v for v in d.others) and any(last[v] == d.layer2[v] for v in d.others)
    q, p = _qi_pair(d, w, 2)
    sizes = []
    for be, bf in sc.batches(evs, flags):
        _process_both(d, q, p, be, bf)
        _same_state(q, p)
        sizes.append(len(be))
    assert sizes[:3] == [1, 16, 17][:len(sizes[:3])] or len(evs) < 34
    if V >= 65:
        assert sizes[:3] == [1, 16, 17] and len(sizes) == 4 and sizes[3] > 17
        assert len(set(q.matrix()[d.hub].tolist())) >= d.K - 1           # the hub's row holds ~K seqs
        assert len(set(q.medians().tolist())) >= 2


@pytest.mark.parametrize("V", WIDTHS)
def test_metric_plan_matches_python_and_passes_2_32(V):
    hub = sc.qi_hub(V)
    d = sc.comb_dag(V, hub=hub, second_layer=True)
    w = sc.heavy_weights(V, hub)
    assert sum(w) == (1 << 31) - 1
    evs, flags, cands = sc.metric_plan(d)
    big = 0
    for cap in sc.METRIC_CAPS:
        q, p = _qi_pair(d, w, cap)
        _process_both(d, q, p, evs, flags)
        _same_state(q, p)
        med = q.medians()
        for c in cands:
            got = q.metric(c, cap, med)
            assert got == p.get_metric_of(c), (cap, c)
            big += got >= 1 << 32
            if cap == 0:
                assert got == 0
    if d.K >= 3:
        assert big >= 1                                                   # a sum whose high half is set
        q, _ = _qi_pair(d, w, 0xFFFFFFFF)
        q.process(evs, flags)
        assert q.metric(d.chain[-1], 0xFFFFFFFF) >= (d.K - 1) * w[hub] >= 1 << 32


def test_fork_metric_has_high_halves_in_two_lanes():
    d = sc.fork3_dag()
    w = sc.FORK3_WEIGHTS
    cap = 0xFFFFFFFF
    q, p = _qi_pair(d, w, cap)
    evs = list(d.sides) + [d.narrow]
    _process_both(d, q, p, evs, [0, 0, 1])
    _same_state(q, p)
    assert list(q.sp) == [2, 2, 2]                                        # the self-parent saw no fork
    got = q.metric(d.wide, cap)
    assert got == p.get_metric_of(d.wide)
    med = q.medians().astype(np.int64)
    per = [(sc.FORK_SEQ - int(med[v])) * w[v] - (2 - int(med[v])) * w[v] for v in (1, 2)]
    assert all(x >= 1 << 32 for x in per) and got >= sum(per)
    assert got >> 32 >= 4                                                 # differences near 2^31 times the weight
