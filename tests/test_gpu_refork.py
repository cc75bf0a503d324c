"""Rollback, then a fork by another creator: every consumer of the branch ->
creator map against the oracle (tests/refork_dags.py, pinned to the oracle by
tests/test_refork_dags.py).

DropNotFlushed takes a fork's branch number back and the next fork, of another
creator, gets it: the branch count is what it was with another map behind it.
Each scenario is driven through the same Add / Flush / Drop sequence as the
oracle -- every consumer uses its tables on the dropped batch first -- and
compared bit for bit with it, and with a fresh handle that only ever saw what
was kept:

* the index: vectors, merged vectors, branch ids, BranchesInfo, all-pairs
  ForklessCause (fc_fk 1 and 0), per-pair ForklessCause over a warm result
  cache, the write-back tables (small_max default and 0) and a handle restored
  from them;
* the emitter's QuorumIndexer (caps 2 and 7), refreshed by ProcessEvent or by
  GetMetricOf alone;
* the abft engine: Build(fork of X) then Process(fork of Y); a claimed batch
  refused at X's fork, then Y's fork;
* column shards, G = 2 in one process, whole and incremental exchange, and
  through ShardedDagIndexer (two gloo ranks on one GPU);
* a whole epoch rolled back at random points and redone in another order,
  with ancestry, fork evidence and MedianTime checked at every flush.

The readers merged later (MedianTime, ancestry, fork evidence, Build without
Add, frame progress) go through the same scenarios in
tests/test_gpu_refork_readers.py.

Before the index counted the generations of that map (lx_index::branch_gen)
the QuorumIndexer, the abft engine and the shard exchange keyed their tables
on the branch count alone, and this module found: QuorumIndexer matrices and
metrics off in 14 of 18 cases (v8_split_lo_hi, metric of event 26: 4 for 3);
frames off after Build(fork of X) in 3 of 9 cases (v4_y_above, event 16:
frame 3 for 4), and in the same 3 an honest claim refused after a batch that
held nothing but X's refused fork (a redone prefix, k = 5, evaluates a frame
at the smaller branch count, which rebuilt the table); and the whole exchange
after drop + re-add of one event packing rows by the row list of the dropped
event -- on the shard that no longer owns the row's branch the plane column
is LX_NONE and the pack read out of bounds.  The index itself passed: its column tables are rebuilt with every
change of the branch set, and the result cache forgot its columns at every
drop.

Measured on an MI355X: the module, 92 tests, 18.6 s in six processes (one
per group); the first case of a process (which starts the device) 1.6-2.0 s,
test_sharded_dag_indexer_after_refork (two more processes) 3.0 s,
test_reshuffled_redo_epoch 0.5 s after the device start (also with the three
readers checked at its 22 flushes), every other case 0.1 s or less.
"""

import multiprocessing as mp
import os
import socket

import numpy as np
import pytest

import refork_dags as rd
from abft_harness import FakeLachesis
from oracle import emitter_oracle as eo
from oracle import rlp
from oracle import vecfc_oracle as vo
from oracle.tdag import Event
from test_gpu_shards import exchange, fc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(rd.VARIANTS)
CAPS = (2, 7)


@pytest.fixture(scope="module")
def lx():
    import lachesis_hip
    return lachesis_hip


def be32(x):
    return int(x).to_bytes(4, "big")


def new_oracle(sc):
    o = vo.Index()
    o.reset(sc.validators, sc.store.get)
    return o


def new_gpu(lx, sc, options=None):
    g = lx.VecfcIndex(engine=lx.Index(options=options)) if options else lx.VecfcIndex()
    g.reset(sc.validators, sc.store.get)
    return g


def add_all(o, g, events):
    for e in events:
        o.add(e)
    g.add_events(events)


def all_pairs(g, ids):
    n = len(ids)
    idx = np.array([g.pos[i] for i in ids], dtype=np.uint32)
    return np.repeat(idx, n), np.tile(idx, n)


def oracle_fc(o, ids):
    return np.array([o.forkless_cause(a, b) for a in ids for b in ids], dtype=np.uint8)


def assert_index_equal(g, o, ids, what):
    for eid in ids:
        assert g.get_highest_before(eid).to_bytes() == o.get_highest_before(eid).to_bytes(), (what, "HB", eid)
        assert g.get_lowest_after(eid).to_bytes() == o.get_lowest_after(eid).to_bytes(), (what, "LA", eid)
        assert g.get_merged_highest_before(eid).to_bytes() == o.get_merged_highest_before(eid).to_bytes(), \
            (what, "merged HB", eid)
        assert g.get_event_branch_id(eid) == o.get_event_branch_id(eid), (what, "branch", eid)
    bi = o.branches_info()
    assert g.branches_info() == (bi.last_seq, bi.creator_idxs, bi.by_creators), what
    qa, qb = all_pairs(g, ids)
    want = oracle_fc(o, ids)
    got = g.ix.forkless_cause_batch(qa, qb)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, "FC batch", ids[bad[0] // len(ids)], ids[bad[0] % len(ids)], int(got[bad[0]]))
    return want


def assert_pairs_equal(g, ids, want, what):
    """lx_forkless_cause pair by pair (the result cache answers what it holds)."""
    n = len(ids)
    for i, a in enumerate(ids):
        for j, b in enumerate(ids):
            assert g.forkless_cause(a, b) == bool(want[i * n + j]), (what, "FC pair", a, b)


INDEX_OPTIONS = {"default": None, "fc_fk0": {"fc_fk": 0}, "small0": {"small_max": 0}}


@pytest.mark.parametrize("opt", sorted(INDEX_OPTIONS))
@pytest.mark.parametrize("name", NAMES)
def test_index_after_refork(lx, name, opt):
    sc = rd.get(name)
    o, g = new_oracle(sc), new_gpu(lx, sc, INDEX_OPTIONS[opt])
    db = {}
    add_all(o, g, sc.P)
    o.flush()
    g.flush(db)
    add_all(o, g, sc.A)
    # X's fork is in every table now: the batch kernel's, the result cache's
    ids_a = [e.id for e in sc.P + sc.A]
    want = assert_index_equal(g, o, ids_a, "A")
    assert_pairs_equal(g, ids_a[-12:], want.reshape(len(ids_a), -1)[-12:, -12:].ravel(), "A")
    o.drop_not_flushed()
    g.drop_not_flushed()
    add_all(o, g, sc.A2)
    # the Puts of the next Flush (vecengine/index.go:78-85)
    wb = g.ix.writeback()
    bi = o.bi
    assert {g.ids[k]: v for k, v in wb["S"].items()} == dict(o.tbl_hb.dirty)
    assert {g.ids[k]: v for k, v in wb["s"].items()} == dict(o.tbl_la.dirty)
    assert {g.ids[k]: v for k, v in wb["b"].items()} == {k: be32(v) for k, v in o.tbl_branch.dirty.items()}
    assert wb["B"] == rlp.encode_branches_info(bi.last_seq, bi.creator_idxs, bi.by_creators)
    add_all(o, g, sc.T)
    ids = [e.id for e in sc.P + sc.A2 + sc.T]
    want = assert_index_equal(g, o, ids, "A2")
    rest = [e.id for e in sc.A2 + sc.T]
    k = len(ids) - len(rest)
    assert_pairs_equal(g, rest, want.reshape(len(ids), -1)[k:, k:].ravel(), "A2")
    assert want[ids.index(sc.ea2.id) * len(ids) + ids.index(sc.xc.id)] == 1
    # a handle that never saw A, and one restored from the written tables
    f = new_gpu(lx, sc, INDEX_OPTIONS[opt])
    f.add_events(sc.P)
    f.flush()
    f.add_events(sc.A2 + sc.T)
    o.flush()
    g.flush(db)
    r = lx.VecfcIndex()
    r.restore(sc.validators, db, sc.store.get)
    qa, qb = all_pairs(g, ids)
    for h, what in ((f, "fresh"), (r, "restored")):
        for eid in ids:
            assert h.get_highest_before(eid).to_bytes() == g.get_highest_before(eid).to_bytes(), (what, eid)
            assert h.get_lowest_after(eid).to_bytes() == g.get_lowest_after(eid).to_bytes(), (what, eid)
            assert h.get_merged_highest_before(eid).to_bytes() == g.get_merged_highest_before(eid).to_bytes(), \
                (what, eid)
        assert h.branches_info() == g.branches_info(), what
        ha, hb = all_pairs(h, ids)
        assert np.array_equal(h.ix.forkless_cause_batch(ha, hb), want), what
    for h in (g, f, r):
        h.ix.close()


# ---------------------------------------------------------------------------- QuorumIndexer

def qi_flags(sc, events):
    return [1 if e.creator - 1 == sc.me else 0 for e in events]


def assert_qi_equal(gq, oq, ids, what):
    for c in CAPS:
        assert np.array_equal(gq[c].get_global_matrix(), np.array(oq[c].get_global_matrix())), (what, c, "matrix")
        assert list(gq[c].get_self_parent_seqs()) == oq[c].get_self_parent_seqs(), (what, c, "self-parent seqs")
        assert list(gq[c].get_global_median_seqs()) == oq[c].get_global_median_seqs(), (what, c, "medians")
        got = list(map(int, gq[c].get_metrics_of(ids)))
        assert got == [oq[c].get_metric_of(x) for x in ids], (what, c, "metrics")


@pytest.mark.parametrize("refresh", ["process", "metric"])
@pytest.mark.parametrize("name", NAMES)
def test_quorum_indexer_after_refork(lx, name, refresh):
    sc = rd.get(name)
    o, g = new_oracle(sc), new_gpu(lx, sc)
    w = sc.validators.weights
    oq = {c: eo.QuorumIndexer(sc.validators, o, eo.capped_metric(w, c)) for c in CAPS}
    gq = {c: lx.emitter.QuorumIndexer(g, c) for c in CAPS}

    def process(events):
        for c in CAPS:
            for e, fl in zip(events, qi_flags(sc, events)):
                oq[c].process_event(e, bool(fl))
            gq[c].process_events(events, qi_flags(sc, events))

    add_all(o, g, sc.P)
    o.flush()
    g.flush()
    process(sc.P)
    add_all(o, g, sc.A)
    process(sc.A)
    assert_qi_equal(gq, oq, [e.id for e in sc.P + sc.A], "A")      # ProcessEvent and GetMetricOf on X's fork
    o.drop_not_flushed()
    g.drop_not_flushed()
    add_all(o, g, sc.A2 + sc.T)
    ids = [e.id for e in sc.P + sc.A2 + sc.T]
    if refresh == "metric":
        # no ProcessEvent since the drop: GetMetricOf alone has to notice
        for c in CAPS:
            got = list(map(int, gq[c].get_metrics_of(ids)))
            assert got == [oq[c].get_metric_of(x) for x in ids], (c, "metrics before ProcessEvent")
    process(sc.A2)
    assert_qi_equal(gq, oq, ids, "A2")
    process(sc.T)
    assert_qi_equal(gq, oq, ids, "T")
    for c in CAPS:
        gq[c].close()
    g.ix.close()


# ---------------------------------------------------------------------------- abft

def copies(events):
    return [Event(e.id, e.creator, e.seq, e.lamport, e.parents, e.name) for e in events]


def wmap(sc):
    return {c + 1: 1 for c in range(sc.V)}


def abft_state(t):
    return dict(blocks=list(t.block_list), last=(t.store.get_epoch(), t.store.last_decided_frame))


@pytest.mark.parametrize("name", NAMES)
def test_abft_build_x_then_process_y(lx, name):
    """Build = Add + frames + DropNotFlushed: X's fork event is built and never
    processed; Y's takes its branch number."""
    sc = rd.get(name, abft=True)
    res = []
    for backend in ("oracle", "gpu"):
        t = FakeLachesis(wmap(sc), backend=backend)
        evs = copies(sc.P + sc.A2 + sc.T)
        built = []
        for e in evs[:len(sc.P)]:
            t.build(e)
            assert t.process(e) is None
        for e in copies(sc.fx):
            t.build(e)
            built.append(e.frame)
        for e in evs[len(sc.P):]:
            t.build(e)
            assert t.process(e) is None
        res.append(dict(frames=[e.frame for e in evs], built=built, **abft_state(t)))
        if backend == "gpu":
            t.lch.close()
    assert res[1]["built"] == res[0]["built"]
    assert res[1]["frames"] == res[0]["frames"]
    assert res[1]["blocks"] == res[0]["blocks"] and res[1]["last"] == res[0]["last"]
    cheaters = {c for b in res[0]["blocks"] for c in b[3]}
    assert sc.X + 1 not in cheaters


@pytest.mark.parametrize("k", [0, 5])
@pytest.mark.parametrize("name", NAMES)
def test_abft_refused_claim_then_fork_of_y(lx, name, k):
    """A claimed batch of k honest events and X's fork event with a wrong
    claim: the batch is refused there and its prefix redone without it (k = 0:
    nothing is redone, so nothing evaluates a frame between the drop and Y's
    fork); the next batch holds Y's fork."""
    sc = rd.get(name, abft=True)
    ref = FakeLachesis(wmap(sc))
    honest = {}
    evs = copies(sc.P + sc.A2 + sc.T)
    for i, e in enumerate(evs):
        if i == len(sc.P):
            for f in copies(sc.fx[:1]):
                ref.build(f)
                honest[f.id] = f.frame
        ref.build(e)
        assert ref.process(e) is None
        honest[e.id] = e.frame
    res = []
    for backend in ("oracle", "gpu"):
        t = FakeLachesis(wmap(sc), backend=backend)
        evs = copies(sc.P + sc.A2 + sc.T)
        head, tail = evs[:len(sc.P) - k], evs[len(sc.P) - k:len(sc.P)]
        for e in head:
            t.build(e)
            assert t.process(e) is None
        batch = tail + copies(sc.fx[:1])
        for e in batch:
            e.frame = honest[e.id]
        batch[-1].frame += 1
        consumed, err = t.process_batch(batch, claimed=True)
        assert consumed == k and err is not None, backend
        rest = evs[len(sc.P):]
        for e in rest:
            e.frame = honest[e.id]
        consumed, err = t.process_batch(rest, claimed=True)
        assert err is None and consumed == len(rest), (backend, consumed, err)
        frames = [t.lch.frame_of(e.id) for e in evs] if backend == "gpu" else [e.frame for e in evs]
        res.append(dict(frames=frames, **abft_state(t)))
        if backend == "gpu":
            t.lch.close()
    assert res[1]["frames"] == res[0]["frames"] == [honest[e.id] for e in evs]
    assert res[1]["blocks"] == res[0]["blocks"] and res[1]["last"] == res[0]["last"]


# ---------------------------------------------------------------------------- column shards

class Shards:
    """G shard handles fed the same events (dense indices in Add order)."""

    def __init__(self, lx, validators, G=2, incremental=False):
        self.lx, self.validators, self.incremental = lx, validators, incremental
        self.shards = [lx.Index(shard_rank=r, shard_count=G) for r in range(G)]
        for ix in self.shards:
            ix.reset(validators.weights)
        self.pos, self.ids, self.n_flushed = {}, [], 0

    def add(self, events):
        creator, seq, off, par = [], [], [0], []
        for e in events:
            creator.append(self.validators.idxs[e.creator])
            seq.append(e.seq)
            par.extend(self.pos[p] for p in e.parents)
            off.append(len(par))
            self.pos[e.id] = len(self.ids)
            self.ids.append(e.id)
        for ix in self.shards:
            ix.add_batch(creator, seq, np.array(off, dtype=np.uint64), par)

    def flush(self):
        for ix in self.shards:
            ix.flush()
        self.n_flushed = len(self.ids)

    def drop(self):
        for ix in self.shards:
            ix.drop_not_flushed()
        for eid in self.ids[self.n_flushed:]:
            del self.pos[eid]
        del self.ids[self.n_flushed:]

    def exchange(self):
        if self.incremental:
            # ShardedIndex.exchange: the rows written since the last committed exchange
            d = np.minimum.reduce([ix.shard_dirty() for ix in self.shards])
            for ix in self.shards:
                ix.shard_dirty_set(d)
        exchange(self.shards)
        if self.incremental:
            for ix in self.shards:
                ix.shard_dirty_commit()

    def fc_all(self, ids):
        idx = np.array([self.pos[i] for i in ids], dtype=np.uint32)
        n = len(ids)
        return fc(self.lx, self.shards, np.repeat(idx, n), np.tile(idx, n))

    def close(self):
        for ix in self.shards:
            ix.close()


def assert_shards_fc(s, o, ids, what):
    s.exchange()
    got, want = s.fc_all(ids), oracle_fc(o, ids)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, "FC", ids[bad[0] // len(ids)], ids[bad[0] % len(ids)], int(got[bad[0]]))


@pytest.mark.parametrize("incremental", [False, True], ids=["whole", "incremental"])
@pytest.mark.parametrize("name", NAMES)
def test_shards_after_refork(lx, name, incremental):
    sc = rd.get(name)
    o = new_oracle(sc)
    s = Shards(lx, sc.validators, 2, incremental)

    def add(events):
        for e in events:
            o.add(e)
        s.add(events)

    add(sc.P)
    o.flush()
    s.flush()
    if incremental:
        s.exchange()
    add(sc.A)
    assert_shards_fc(s, o, [e.id for e in sc.P + sc.A], "A")
    o.drop_not_flushed()
    s.drop()
    add(sc.A2)
    assert_shards_fc(s, o, [e.id for e in sc.P + sc.A2], "A2")
    add(sc.T)
    assert_shards_fc(s, o, [e.id for e in sc.P + sc.A2 + sc.T], "T")
    s.close()


def _dag_indexer_worker(rank, world, port, q, names):
    import sys
    sys.path[:0] = [ROOT, os.path.join(ROOT, "lachesis-base_amd"), os.path.join(ROOT, "tests")]
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    bad = []
    try:
        import lachesis_hip as lx
        from lachesis_hip.shard import ShardedDagIndexer, ShardedIndex
        for name in names:
            sc = rd.get(name)
            o = new_oracle(sc)
            ix = lx.Index(device=0, shard_rank=rank, shard_count=world)
            sdi = ShardedDagIndexer(ShardedIndex(ix, device=torch.device("cuda", 0)))
            sdi.reset(sc.validators, sc.store.get)

            def add(events):
                for e in events:
                    o.add(e)
                    sdi.add(e)

            def check(ids, pairs, what):
                for eid in ids:
                    for fn in ("get_highest_before", "get_lowest_after", "get_merged_highest_before"):
                        if getattr(sdi, fn)(eid).to_bytes() != getattr(o, fn)(eid).to_bytes():
                            bad.append((name, what, fn, eid))
                for a, b in pairs:
                    if sdi.forkless_cause(a, b) != o.forkless_cause(a, b):
                        bad.append((name, what, "FC", a, b))

            add(sc.P)
            o.flush()
            sdi.flush()
            add(sc.A)
            fx = sc.fx[0].id
            check([e.id for e in sc.A[:6]], [(e.id, fx) for e in sc.A[:6]] + [(fx, e.id) for e in sc.P[-6:]], "A")
            o.drop_not_flushed()
            sdi.drop_not_flushed()
            add(sc.A2)
            check([e.id for e in sc.A2[:3]], [(sc.A2[0].id, e.id) for e in sc.P[-6:]], "A2")
            add(sc.T)
            core = [sc.fy[0].id, sc.xc.id, sc.ea.id, sc.ea2.id, sc.eb.id]
            check(core, [(a, b) for a in core for b in core + [e.id for e in sc.P[-4:]]], "T")
            ix.close()
        q.put((rank, bad[:5], None))
    except Exception as e:   # report instead of hanging the other rank's queue read
        import traceback
        q.put((rank, bad[:5], repr(e) + traceback.format_exc()[-1500:]))
    finally:
        dist.destroy_process_group()


def test_sharded_dag_indexer_after_refork():
    """ShardedDagIndexer.add / drop_not_flushed / getters / forkless_cause on
    two gloo ranks sharing the GPU: the per-event cadence, X and Y in different
    shards."""
    names = ["v8_split_lo_hi", "v8_split_z", "v4_y_below", "v8_split_hi_lo"]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = [ctx.Process(target=_dag_indexer_worker, args=(r, 2, port, q, names)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=300) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert all(not bad and err is None for _, bad, err in res), res


# ---------------------------------------------------------------------------- reshuffled redo

def test_reshuffled_redo_epoch(lx):
    """Index, QuorumIndexer and shards over an epoch that is rolled back to the
    last flush at random points and redone in another parents-first order; at
    every flush ancestry, fork evidence and MedianTime against their models
    over the current order."""
    import ancestry_model as am
    import fork_evidence_model as fm
    import median_time_model as mm
    validators, store, ops = rd.reshuffled()
    o = vo.Index()
    o.reset(validators, store.get)
    g = lx.VecfcIndex()
    g.reset(validators, store.get)
    s = Shards(lx, validators, 2, True)
    w = validators.weights
    oq = eo.QuorumIndexer(validators, o, eo.capped_metric(w, 2))
    gq = lx.emitter.QuorumIndexer(g, 2)
    anc, mt = lx.AncestryIndex(g), lx.MedianTimeIndex(g)
    times = dict(zip(sorted(store), mm.event_times(len(store), 9)))     # by event id, whatever the order
    me = 0
    for step, op in enumerate(ops):
        if op[0] == "flush":
            order = [store[i] for i in g.ids]
            m = am.Model(validators, order)
            n = m.n
            got = anc.observes_dense(np.repeat(np.arange(n), n), np.tile(np.arange(n), n)).reshape(n, n)
            assert np.array_equal(got, m.observes_matrix()), step
            assert anc.cheaters_dense(np.arange(n)) == [fm.cheaters(m, h) for h in range(n)], step
            assert mt.num_times() == n
            d = mm.derived_of(validators, order, [times[i] for i in g.ids])
            for dflt in (0, 1 << 40):
                want = [d.median(*d.merged(i)[:2], dflt) for i in range(n)]
                assert [int(x) for x in mt.median_time(g.ids, dflt)] == want, (step, dflt)
            o.flush()
            g.flush()
            s.flush()
            continue
        if op[0] == "drop":
            o.drop_not_flushed()
            g.drop_not_flushed()
            s.drop()
            continue
        part = op[1]
        add_all(o, g, part)
        s.add(part)
        mt.set_times(part, [times[e.id] for e in part])      # (a drop forgets the times of what it drops)
        flags = [1 if validators.idxs[e.creator] == me else 0 for e in part]
        for e, fl in zip(part, flags):
            oq.process_event(e, bool(fl))
        gq.process_events(part, flags)
        new = [e.id for e in part]
        bi = o.branches_info()
        assert g.branches_info() == (bi.last_seq, bi.creator_idxs, bi.by_creators), step
        for eid in new:
            assert g.get_highest_before(eid).to_bytes() == o.get_highest_before(eid).to_bytes(), (step, eid)
            assert g.get_merged_highest_before(eid).to_bytes() == o.get_merged_highest_before(eid).to_bytes(), \
                (step, eid)
            assert g.get_event_branch_id(eid) == o.get_event_branch_id(eid), (step, eid)
        # ForklessCause(a, b) for the new a: it never changes once a is indexed
        qa = np.repeat(np.array([g.pos[i] for i in new], dtype=np.uint32), len(g.ids))
        qb = np.tile(np.arange(len(g.ids), dtype=np.uint32), len(new))
        want = np.array([o.forkless_cause(a, b) for a in new for b in g.ids], dtype=np.uint8)
        assert np.array_equal(g.ix.forkless_cause_batch(qa, qb), want), step
        assert g.ids == s.ids
        s.exchange()
        assert np.array_equal(fc(lx, s.shards, qa, qb), want), step
        assert np.array_equal(gq.get_global_matrix(), np.array(oq.get_global_matrix())), step
        assert list(gq.get_global_median_seqs()) == oq.get_global_median_seqs(), step
        assert list(map(int, gq.get_metrics_of(new))) == [oq.get_metric_of(x) for x in new], step
    for eid in g.ids:
        assert g.get_lowest_after(eid).to_bytes() == o.get_lowest_after(eid).to_bytes(), eid
    assert any(fm.cheaters(m, h) for h in range(m.n))
    gq.close()
    anc.close()
    mt.close()
    g.ix.close()
    s.close()
