"""MedianTime on the GPU (include/lachesis_mediantime.h, lachesis_hip.mediantime)
against the derived CPU model (tests/median_time_model.py, itself pinned to
the carried vecmt form by tests/test_median_time_model.py): merged times and
medians bit-exact for every event, the maximum width, rollback, times set
ahead of Add, epoch reset, error paths, restart, and the queries from inside
the abft engine's block callbacks."""

import ctypes

import numpy as np
import pytest

import median_time_model as mm
from abft_harness import FakeLachesis, node_ids, topo_shuffle
from oracle import pos, tdag
from oracle.tdag import SplitMix64

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -1, -4


@pytest.fixture(scope="module")
def lx():
    import lachesis_hip
    return lachesis_hip


def _index(lx, validators, events):
    ix = lx.VecfcIndex()
    ix.reset(validators)
    ix.add_events(events)
    return ix


def _expected(d, n, rows=None):
    """Model's (merged times [n x V], medians per default) of events `rows`."""
    rows = range(n) if rows is None else rows
    merged, med = [], {dflt: [] for dflt in mm.DEFAULTS}
    for i in rows:
        kind, time, _ = d.merged(i)
        merged.append(time)
        for dflt in mm.DEFAULTS:
            med[dflt].append(d.median(kind, time, dflt))
    return np.array(merged, dtype=np.uint64), {k: np.array(v, dtype=np.uint64) for k, v in med.items()}


def _check_all(mt, d, events):
    ids = [e.id for e in events]
    merged, med = _expected(d, len(events))
    assert np.array_equal(mt.merged_times(ids), merged)
    for dflt in mm.DEFAULTS:
        assert np.array_equal(mt.median_time(ids, dflt), med[dflt]), dflt
    for k, eid in enumerate(ids[:8]):                       # one call per event
        assert np.array_equal(mt.merged_times([eid])[0], merged[k]), k
        for dflt in mm.DEFAULTS:
            assert int(mt.median_time([eid], dflt)[0]) == int(med[dflt][k]), (k, dflt)
    return med


@pytest.mark.parametrize("shape,wk", [(s, "skewed") for s in mm.SHAPES] + [
    ((9, 20, 3, 9, 4, 7), "equal"),
    ((1000, 3, 10, 0, 0, 5), "zipf"),           # BASELINE configs[4] scale: V = 1000, Zipf stakes
])
def test_median_time_matches_model(lx, shape, wk):
    V = shape[0]
    w = {"skewed": mm.skewed(V), "equal": [1] * V, "zipf": [(1 << 20) // (i + 1) for i in range(V)]}[wk]
    validators, events, times = mm.build_shape(shape, w)
    d = mm.derived_of(validators, events, times)
    ix = _index(lx, validators, events)
    mt = lx.MedianTimeIndex(ix)
    mt.set_times(events, times)
    assert mt.num_times() == len(events)
    med = _check_all(mt, d, events)
    if V > 1:
        assert len({int(x) for m in med.values() for x in m}) >= 2


def test_maximum_width(lx):
    """V = 8192 (eight validators per thread of the widest workgroup); one
    more is refused at create."""
    V = 8192
    nodes, events = tdag.rand_fork_dag(V, 2, 4, seed=8)
    validators = pos.Validators.equal(nodes, 1)
    times = mm.event_times(len(events), 8)
    d = mm.derived_of(validators, events, times)
    ix = _index(lx, validators, events)
    mt = lx.MedianTimeIndex(ix)
    mt.set_times_dense(0, times)
    last = list(range(len(events) - 64, len(events)))
    ids = [events[i].id for i in last]
    for dflt in (1020,) + mm.DEFAULTS:
        exp = [d.median(*d.merged(i)[:2], dflt) for i in last]
        assert [int(x) for x in mt.median_time(ids, dflt)] == exp, dflt
    merged, _ = _expected(d, 0, last[-2:])
    assert np.array_equal(mt.merged_times(ids[-2:]), merged)

    big = lx.Index()
    big.reset([1] * (V + 1))
    h = ctypes.c_void_p()
    assert big.L.lx_mt_create(big.h, ctypes.byref(h)) == ERR_ARG


def _raw_median(mt, ev):
    a = np.array(ev, dtype=np.uint32)
    out = np.zeros(len(a), dtype=np.uint64)
    rc = mt.L.lx_mt_median_time(mt.h, len(a), a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), 5,
                                out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)))
    return rc, mt.L.lx_mt_last_error(mt.h).decode()


def test_rollback_forgets_dropped_times(lx):
    validators, events, times = mm.build_shape((12, 30, 4, 3, 5, 2))
    k, m = 150, 260
    ix = _index(lx, validators, events[:k])
    mt = lx.MedianTimeIndex(ix)
    mt.set_times(events[:k], times[:k])
    ix.flush()
    # more events, and times set ahead beyond them
    ix.add_events(events[k:m])
    mt.set_times_dense(k, times[k:m] + [7] * 20)
    assert mt.num_times() == m + 20
    ix.drop_not_flushed()
    assert mt.num_times() == k
    rc, msg = _raw_median(mt, [k])
    assert rc == ERR_STATE and "time not set" in msg
    # other events at those indices, other times
    again = topo_shuffle(events[k:], SplitMix64(5))
    assert [e.id for e in again[:m - k]] != [e.id for e in events[k:m]]
    new_times = times[:k] + mm.event_times(len(again), 77)
    ix.add_events(again)
    mt.set_times(again, new_times[k:])
    order = events[:k] + again
    _check_all(mt, mm.derived_of(validators, order, new_times), order)
    # a second rollback to the same flushed count
    ix.drop_not_flushed()
    assert mt.num_times() == k


def test_times_set_ahead_of_add(lx):
    validators, events, times = mm.build_shape((40, 12, 6, 8, 4, 3))
    ids = [e.id for e in events]
    ix = lx.VecfcIndex()
    ix.reset(validators)
    mt = lx.MedianTimeIndex(ix)
    mt.set_times(events, times)                              # nothing added yet
    assert mt.num_times() == len(events) and ix.ix.num_events() == 0
    ix.add_events(events)
    ahead = {dflt: mt.median_time(ids, dflt) for dflt in mm.DEFAULTS}
    ahead_rows = mt.merged_times(ids)
    mt2 = lx.MedianTimeIndex(ix)
    mt2.set_times(events, times)                             # after Add
    for dflt in mm.DEFAULTS:
        assert np.array_equal(mt2.median_time(ids, dflt), ahead[dflt])
    assert np.array_equal(mt2.merged_times(ids), ahead_rows)
    _check_all(mt, mm.derived_of(validators, events, times), events)


def test_index_reset_leaves_no_times(lx):
    validators, events, times = mm.build_shape((7, 25, 3, 0, 0, 1))
    ix = _index(lx, validators, events)
    mt = lx.MedianTimeIndex(ix)
    mt.set_times(events, times)
    ix.flush()
    ix.reset(validators)                                     # lx_reset, not lx_mt_reset
    assert mt.num_times() == 0
    # a smaller validator set in the next epoch is taken over with it
    v2, ev2, t2 = mm.build_shape((4, 6, 3, 0, 0, 2))
    ix.reset(v2)
    ix.add_events(ev2)
    ix.flush()
    rc, msg = _raw_median(mt, [0])
    assert rc == ERR_STATE and "time not set" in msg
    mt.set_times(ev2, t2)
    _check_all(mt, mm.derived_of(v2, ev2, t2), ev2)
    mt.reset()
    assert mt.num_times() == 0


def test_error_paths(lx):
    validators, events, times = mm.build_shape((7, 25, 3, 0, 0, 1))
    n = len(events)
    ix = _index(lx, validators, events)
    mt = lx.MedianTimeIndex(ix)
    # a hole: nothing held, times from event 3 on
    with pytest.raises(lx.LxError) as ei:
        mt.set_times_dense(3, times[3:])
    assert ei.value.code < 0 and "hole" in str(ei.value)
    assert mt.num_times() == 0
    # time not set: a prefix only
    mt.set_times_dense(0, times[:10])
    rc, msg = _raw_median(mt, [2, 10])
    assert rc == ERR_STATE and "time not set" in msg
    with pytest.raises(lx.LxError) as ei:
        mt.merged_times_dense([n - 1])
    assert ei.value.code == ERR_STATE
    # unknown event: times run ahead of the events
    mt.set_times_dense(10, times[10:] + [1, 2, 3])
    rc, msg = _raw_median(mt, [0, n + 1])
    assert rc == ERR_ARG and "unknown event" in msg
    rc, msg = _raw_median(mt, [n + 3])
    assert rc == ERR_STATE
    # earlier entries may be overwritten
    mt.set_times_dense(0, times[:5])
    _check_all(mt, mm.derived_of(validators, events, times), events)
    # a column shard holds partial rows
    sh = lx.Index(shard_rank=0, shard_count=2)
    sh.reset(validators.weights)
    h = ctypes.c_void_p()
    assert sh.L.lx_mt_create(sh.h, ctypes.byref(h)) == ERR_STATE


def test_restart_set_times_again(lx):
    validators, events, times = mm.build_shape((12, 30, 4, 3, 5, 2))
    ids = [e.id for e in events]
    store = {e.id: e for e in events}
    ix = _index(lx, validators, events)
    mt = lx.MedianTimeIndex(ix)
    mt.set_times(events, times)
    db = {}
    ix.flush(db)
    want = {dflt: mt.median_time(ids, dflt) for dflt in mm.DEFAULTS}
    want_rows = mt.merged_times(ids)

    ix2 = lx.VecfcIndex()
    ix2.reset(validators)
    mt2 = lx.MedianTimeIndex(ix2)
    mt2.set_times_dense(0, [9] * 40)                         # of no event of the load
    ix2.restore(validators, db, store.get)
    assert mt2.num_times() == 0                              # nothing is persisted
    assert ix2.ix.at_least_one_fork()
    mt2.set_times(events, times)                             # by event id: the load's dense order is its own
    for dflt in mm.DEFAULTS:
        assert np.array_equal(mt2.median_time(ids, dflt), want[dflt])
    assert np.array_equal(mt2.merged_times(ids), want_rows)


class _TimedLachesis(FakeLachesis):
    """The harness's TestLachesis whose BeginBlock asks the block's time."""

    mt = None

    def _begin_block(self, block):
        if self.mt is not None:
            a = self.lch.pos[block.atropos]
            self.asked.append((self.store.get_epoch(), a, int(self.mt.median_time_dense([a], self.default)[0]),
                               self.mt.merged_times_dense([a])[0]))
        return super()._begin_block(block)


def test_block_time_in_abft_callbacks(lx):
    """BeginBlock asks MedianTime(atropos); the sealing block's value cannot be
    fetched later (the index is reset right after its EndBlock)."""
    weights = [1, 2, 1, 2, 1, 2, 1, 2, 1, 2]
    nodes = node_ids(len(weights), seed=11)
    _, evs = tdag.rand_fork_dag(len(nodes), 60, 5, cheaters=0, forks_count=10, node_ids=nodes, rng=SplitMix64(11))
    t = _TimedLachesis(dict(zip(nodes, weights)), backend="gpu")
    t.asked, t.default = [], 1010
    end_rows = []

    def apply_block(block):                                  # EndBlock: seal at frame 3 (test_gpu_abft's set-up)
        end_rows.append(int(t.mt.median_time_dense([t.lch.pos[block.atropos]], t.default)[0]))
        if t.store.last_decided_frame + 1 == 3:
            return t.store.get_validators()
        return None
    t.apply_block = apply_block

    class _Dagi:                                             # what MedianTimeIndex needs of its index
        ix, validators = t.lch.ix, t.lch.validators
    t.mt = lx.mediantime.MedianTimeIndex(_Dagi)
    times = mm.event_times(len(evs), 11)
    t.mt.set_times_dense(0, times)                           # ahead of the batch's Add
    consumed, err = t.process_batch(evs, claimed=False)
    assert err is None and consumed < len(evs) and t.store.get_epoch() == 2
    assert len(t.asked) == 3 and [b[1] for b in t.block_list] == [1, 2, 3]

    validators = pos.Validators(dict(zip(nodes, weights)))
    d = mm.derived_of(validators, evs, times)
    for k, (epoch, a, got, row) in enumerate(t.asked):
        kind, time, _ = d.merged(a)
        assert epoch == 1 and got == d.median(kind, time, t.default), k
        assert np.array_equal(row, time), k
        assert end_rows[k] == got
    assert len({a for _, a, _, _ in t.asked}) == 3
    assert t.mt.num_times() == 0                             # the seal reset the index
