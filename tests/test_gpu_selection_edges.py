"""The stake-weighted selection kernels at chosen values and widths, against
the numpy models of tests/selection_cases.py (pinned on the CPU by
tests/test_selection_cases.py).  Bit-exact throughout.

MedianTime (k_mt<E>, lx_mediantime.hip): every launch configuration between
a partial wave and eight validators per thread, with times that walk the bit
descent through every bit at the exact weight edge.  The widths and what
launch_mt makes of them:

    63, 64, 65   k_mt<1>: partial wave, whole wave, one entry past a wave
    1024         k_mt<1> at its largest block
    1025, 2048   k_mt<2>: one entry in the second slot, full
    2049, 3073   k_mt<4>: E = 3 (a padding slot), E = 4 with one entry in the last
    4097, 7169   k_mt<8>: E = 5 (three padding slots), E = 8 with one entry in the last

QuorumIndexer (k_qi_median, k_qi_metric, lx_emitter.hip): every sort width
P = 64..8192, subsets that sit on the quorum, batches around kQiInline, and
metric sums with the high half set.
"""

import ctypes
import types

import numpy as np
import pytest

import median_time_model as mm
import selection_cases as sc
from oracle import pos, tdag

pytestmark = pytest.mark.gpu

ERR_ARG = -1
MT_WIDTHS = [63, 64, 65, 1024, 1025, 2048, 2049, 3073, 4097, 7169]
QI_WIDTHS = [1, 64, 65, 129, 257, 513, 1025, 2049, 4097]


@pytest.fixture(scope="module")
def lx():
    import lachesis_hip
    return lachesis_hip


class _Dagi:
    """What MedianTimeIndex / QuorumIndexer need of their index: dense events
    are their own ids."""

    def __init__(self, lx, w, arrays):
        self.ix = lx.Index()
        self.ix.reset(w)
        self.ix.add_batch(*arrays)
        self.validators = types.SimpleNamespace(weights=list(w))
        self.ids = range(len(arrays[0]))

    def _idx(self, ev):
        return int(ev)


# ----------------------------------------------------------------------------
# MedianTime

def _run_mt(mt, q, cases):
    """Every case through the kernel: the median and the merged row."""
    assert cases
    for c in cases:
        mt.set_times_dense(0, q.event_times(c.t))            # overwrites the sources' times
        got = int(mt.median_time_dense([q.ev], c.default)[0])
        want = q.median(c.t, c.default)
        assert got == want, (q.ev, c, hex(got), hex(want))
        if c.expect is not None:
            assert got == c.expect, (q.ev, c)
        assert np.array_equal(mt.merged_times_dense([q.ev])[0], q.merged_row(c.t)), (q.ev, c)


@pytest.fixture(scope="module", params=MT_WIDTHS)
def mt_env(lx, request):
    V = request.param
    d = sc.comb_dag(V)
    w = sc.mixed_weights(V)
    model = sc.MtModel(w, d.arrays())
    mt = lx.MedianTimeIndex(_Dagi(lx, w, d.arrays()))
    return d, model, mt


def test_mt_bit_ladder(mt_env):
    """c_K observes everyone: for every bit b two values that first differ at b,
    the low group at half - 1 (the high value), half and half + 1 (the low)."""
    d, model, mt = mt_env
    q = model.query(d.chain[-1])
    cases = sc.ladder_cases(q, seed=d.V)
    assert len(cases) == 192
    _run_mt(mt, q, cases)


def test_mt_spread_on_three_queries(mt_env):
    """Uniform, windowed, equal and extreme times on c_K, on a mid-chain event
    (the unobserved rest weighs in at the default time) and on a root."""
    d, model, mt = mt_env
    assert d.K >= 2
    for ev in (d.chain[-1], d.chain[d.K // 2 - 1], d.V // 2):
        q = model.query(ev)
        _run_mt(mt, q, sc.spread_cases(q))
    # all three in one launch, one default: blockIdx picks the row
    top = model.query(d.chain[-1])
    case = sc.spread_cases(top)[0]
    mt.set_times_dense(0, top.event_times(case.t))
    evs = [d.chain[-1], d.chain[d.K // 2 - 1], d.V // 2]
    t = top.event_times(case.t)
    want = []
    for ev in evs:
        q = model.query(ev)
        want.append(q.median(t[q.src], case.default))
    assert [int(x) for x in mt.median_time_dense(evs, case.default)] == want


@pytest.mark.parametrize("V", [65, 1025])
def test_mt_dominant_validator(lx, V):
    d = sc.comb_dag(V)
    w = sc.dominant_weights(V)
    model = sc.MtModel(w, d.arrays())
    mt = lx.MedianTimeIndex(_Dagi(lx, w, d.arrays()))
    q = model.query(d.chain[-1])
    _run_mt(mt, q, sc.dominant_cases(q))
    _run_mt(mt, q, sc.spread_cases(q))


def test_mt_half_zero(lx):
    """half == 0: the smallest time of all pairs -- V = 1 with weight 1, and an
    honest weight of 1 beside two cheaters, whose zeros count."""
    d = sc.comb_dag(1)
    model = sc.MtModel([1], d.arrays())
    mt = lx.MedianTimeIndex(_Dagi(lx, [1], d.arrays()))
    for ev in range(len(d)):
        q = model.query(ev)
        assert q.half == 0
        _run_mt(mt, q, sc.spread_cases(q))
    f = sc.fork3_dag()
    model = sc.MtModel(sc.FORK3_WEIGHTS, f.arrays())
    dagi = _Dagi(lx, sc.FORK3_WEIGHTS, f.arrays())
    assert dagi.ix.num_branches() == 5
    mt = lx.MedianTimeIndex(dagi)
    q = model.query(f.wide)
    assert q.half == 0 and q.honest == 1
    cases = sc.spread_cases(q)
    _run_mt(mt, q, cases)
    mt.set_times_dense(0, q.event_times(cases[0].t))
    assert int(mt.median_time_dense([f.wide], 9)[0]) == 0
    q = model.query(f.narrow)
    assert q.half == 5
    _run_mt(mt, q, sc.spread_cases(q))


@pytest.mark.parametrize("shape", [(1025, 3, 8, 5, 2), (2049, 2, 8, 5, 2), (2049, 3, 8, 5, 2)])
def test_mt_fork_dags_with_random_times(lx, shape):
    """Seeded DAGs with uniform random 64-bit times through k_mt<2> and
    k_mt<4>.  A cheater forks at its third event at the earliest, so the
    shapes with three events per node take the fork path (cheat_of, marks,
    weightless entries); the one with two has the width alone.  The last 1536
    events are asked: the fork-observing ones are among them."""
    V, epn, P, cheaters, forks = shape
    nodes, events = tdag.rand_fork_dag(V, epn, P, cheaters, forks)
    validators = pos.Validators(dict(zip(nodes, sc.mixed_weights(V))))
    rng = np.random.default_rng(V)
    times = rng.integers(0, 1 << 64, size=len(events), dtype=np.uint64)
    d = mm.derived_of(validators, events, times.tolist())
    dagi = _Dagi(lx, validators.weights, tdag.to_dense(events, validators))
    mt = lx.MedianTimeIndex(dagi)
    mt.set_times_dense(0, times)
    evs = list(range(len(events) - 1536, len(events)))
    rows = [d.merged(i) for i in evs]
    if epn >= 3:
        assert dagi.ix.num_branches() == V + cheaters
        assert sum(int((kind == mm.FORK).sum()) for kind, _, _ in rows) >= 100
    for dflt in (5, int(rng.integers(0, 1 << 64, dtype=np.uint64))):
        want = np.array([d.median(kind, time, dflt) for kind, time, _ in rows], dtype=np.uint64)
        assert np.array_equal(mt.median_time_dense(evs, dflt), want), dflt
    assert np.array_equal(mt.merged_times_dense(evs[-64:]), np.array([r[1] for r in rows[-64:]], dtype=np.uint64))


# ----------------------------------------------------------------------------
# QuorumIndexer

def _process(q, evs, flags):
    ev = np.ascontiguousarray(evs, dtype=np.uint32)
    fl = np.ascontiguousarray(flags, dtype=np.uint8)
    assert len(ev) == len(fl)
    if len(ev):
        q._chk(q.L.lx_qi_process_events(q.h, len(ev), ev.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                        fl.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))))


def _same_state(q, model, med=None):
    assert np.array_equal(q.get_global_matrix(), model.matrix())
    assert np.array_equal(q.get_self_parent_seqs(), model.sp)
    med = model.medians() if med is None else med
    assert np.array_equal(q.get_global_median_seqs(), med)
    return med


@pytest.fixture(scope="module", params=QI_WIDTHS)
def qi_env(lx, request):
    """One comb with its second layer per width; the stakes of a case class
    are set by a reset of the same index."""
    V = request.param
    d = sc.comb_dag(V, hub=sc.qi_hub(V), second_layer=True)
    return d, {}


def _qi_pair(lx, env, stakes, cap):
    """(device QuorumIndexer, model, weights) over the comb with the stakes
    named; the index and the oracle are built once per stake vector of a width."""
    d, cache = env
    if stakes not in cache:
        cache.clear()                                        # one index of a width at a time
        w = sc.mixed_weights(d.V) if stakes == "mixed" else sc.heavy_weights(d.V, d.hub)
        cache[stakes] = (w, _Dagi(lx, w, d.arrays()), sc.oracle_of(w, d.arrays()))
    w, dagi, o = cache[stakes]
    return lx.emitter.QuorumIndexer(dagi, cap), sc.QiModel(w, o, d.creator), w


def test_qi_quorum_edge(lx, qi_env):
    """Creator subsets of weight Q - 1, Q, Q + 1 that all observe root u, from
    the start, the end and the middle of the index range: row u's median is 0
    below the quorum and >= 1 at it."""
    d, _ = qi_env
    q, model, w = _qi_pair(lx, qi_env, "mixed", 2)
    cases = sc.quorum_edge_cases(d, w)
    assert len(cases) == (9 if d.V > 1 else 6)
    Q = sc.quorum_of(w)
    assert q.dagi.ix.quorum() == Q
    for name, evs, u, S, target in cases:
        q.reset()
        model.reset()
        _process(q, evs, [0] * len(evs))
        model.process(evs, [0] * len(evs))
        med = _same_state(q, model)
        assert (int(med[u]) == 0) if target < Q else (int(med[u]) >= 1), name


def test_qi_whole_matrix(lx, qi_env):
    """Every second-layer event with chain events and roots interleaved, self
    flags on the hub, in batches of 1, 16, 17 and the rest."""
    d, _ = qi_env
    q, model, _ = _qi_pair(lx, qi_env, "mixed", 2)
    evs, flags = sc.whole_matrix_plan(d, d.hub)
    for be, bf in sc.batches(evs, flags):
        _process(q, be, bf)
        model.process(be, bf)
        med = _same_state(q, model)
    for cap in (2, 7):
        q.cap = cap
        assert [int(x) for x in q.get_metrics_of(d.chain)] == [model.metric(c, cap, med) for c in d.chain], cap


def test_qi_metric_high_half(lx, qi_env):
    """heavy stakes on the hub (total 2^31 - 1): the chain's metrics pass 2^32
    wherever the chain is long enough, for caps 0, 2 and 0xFFFFFFFF."""
    d, _ = qi_env
    evs, flags, cands = sc.metric_plan(d)
    big = 0
    for cap in sc.METRIC_CAPS:
        q, model, w = _qi_pair(lx, qi_env, "heavy", cap)
        assert sum(w) == (1 << 31) - 1
        _process(q, evs, flags)
        model.process(evs, flags)
        med = _same_state(q, model)
        want = [model.metric(c, cap, med) for c in cands]
        assert [int(x) for x in q.get_metrics_of(cands)] == want, cap
        big += sum(x >= 1 << 32 for x in want)
    assert big >= 1 or d.K < 3


def test_qi_fork_metric(lx):
    """A candidate that sees two forks its self-parent does not, uncapped:
    differences near 2^31 times the weight, high halves in two lanes."""
    d = sc.fork3_dag()
    w = sc.FORK3_WEIGHTS
    dagi, o = _Dagi(lx, w, d.arrays()), sc.oracle_of(w, d.arrays())
    for cap in sc.METRIC_CAPS:
        q, model = lx.emitter.QuorumIndexer(dagi, cap), sc.QiModel(w, o, d.creator)
        evs = list(d.sides) + [d.narrow]
        _process(q, evs, [0, 0, 1])
        model.process(evs, [0, 0, 1])
        med = _same_state(q, model)
        cands = [d.wide, d.narrow, 0]
        want = [model.metric(c, cap, med) for c in cands]
        assert [int(x) for x in q.get_metrics_of(cands)] == want, cap
        if cap == 0xFFFFFFFF:
            assert want[0] >> 32 >= 4


def test_qi_maximum_width(lx):
    """V = 8192, P = 8192: 65536 B of sort keys beside the kernel's static
    LDS.  The comb's roots, then c_1, under heavy stakes (the hub alone has the
    quorum): medians of 64 sampled rows and c_1's metric.  One validator more
    is refused at create."""
    V = 8192
    hub = sc.qi_hub(V)
    d = sc.comb_dag(V, hub=hub)
    w = sc.heavy_weights(V, hub)
    n = V + 1                                                # the roots and c_1
    cr, sq, off, par = d.arrays()
    arrays = (cr[:n], sq[:n], off[:n + 1], par[:int(off[n])])
    dagi, o = _Dagi(lx, w, arrays), sc.oracle_of(w, arrays)
    q, model = lx.emitter.QuorumIndexer(dagi, 2), sc.QiModel(w, o, d.creator)
    c1 = d.chain[0]
    assert c1 == V
    rows = sorted(set(np.random.default_rng(8).integers(0, V, size=51).tolist()) | set(d.others[:11]) | {hub, V - 1})
    assert len(rows) <= 64

    def sampled():
        """The model's medians of `rows`; whatever c_1 observes is among them,
        so its metric reads no other."""
        med = np.zeros(V, dtype=np.uint32)
        med[rows] = model.medians(rows)
        assert np.array_equal(q.get_global_median_seqs()[rows], med[rows])
        return med

    roots, flags = list(range(V)), [1 if v == hub else 0 for v in range(V)]
    _process(q, roots, flags)
    model.process(roots, flags)
    med = sampled()
    assert med[hub] == 1 and int(med.sum()) == 1
    for cap in (2, 0xFFFFFFFF):
        q.cap = cap
        want = model.metric(c1, cap, med)
        assert want == w[hub] + 11 and int(q.get_metric_of(c1)) == want, cap

    _process(q, [c1], [0])
    model.process([c1], [0])
    med = sampled()
    assert med[hub] == 2 and int((med == 1).sum()) == 11
    assert np.array_equal(q.get_self_parent_seqs(), model.sp)
    assert int(q.get_metric_of(c1)) == model.metric(c1, 0xFFFFFFFF, med)

    big = lx.Index()
    big.reset([1] * (V + 1))
    h = ctypes.c_void_p()
    assert big.L.lx_qi_create(big.h, ctypes.byref(h)) == ERR_ARG
