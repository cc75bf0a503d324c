"""Rollback, then a fork by another creator (tests/refork_dags.py): the readers
of the index's branch tables that were merged after tests/test_gpu_refork.py,
driven through the same sequence -- a flushed prefix P, a batch A in which X
forks, DropNotFlushed, a batch A2 in which Y forks and gets X's branch number,
a tail T -- and compared bit for bit with their CPU models over exactly the
events present.  tests/test_refork_dags.py shows for each reader and each of
the nine scenarios a query whose answer differs under the map of A.

* MedianTime (lx_mt_*): the cheater lists, the (branch, seq) -> event table,
  the times of dropped events; medians of every event under the defaults 0 and
  2^40 and every merged row, against median_time_model.Derived;
* ancestry (lx_anc_observes, lx_anc_confirm): all pairs, confirm calls with
  heads in the dropped batch and after it, the label table cut at the
  rollback, against ancestry_model.Model;
* fork evidence (lx_anc_fork_pairs, lx_anc_cheaters): every (head, creator),
  the lists of all heads in one call, nothing of X after the drop, against
  fork_evidence_model;
  each of the three at three points (after A on the unflushed events, after
  drop + A2, after T), small_max default and 0, and at the end against a
  handle that never saw A and one restored from the written-back tables;
* Build without Add and frame progress in the abft engine
  (lx_abft_build_frames, lx_abft_build_progress, lx_abft_event_progress): on
  the two drives of test_gpu_refork.py that roll back inside the engine --
  Build(fork of X) then Process(fork of Y), and a claimed batch refused at X's
  fork -- every event that continues its branch's tip asked as a candidate
  before it is processed, all tips' candidates in one call, the candidates
  that must be refused right after the rollback, the progress sums and pair
  stakes against progress_model, and the surroundings of the calls unchanged;
  under three feedings: default options (the small path's incremental host
  mirror), small_max = 0 (every batch on the walker path: the mirror re-read
  from the device before each call), and P as one walker batch followed by
  per-event small batches (the re-read mirror kept up incrementally, and
  rolled back).

Found: nothing.  The stale answers that tests/test_refork_dags.py computes
(v4_y_below: MedianTime(ea) 1085 for 1106; observes(eb, fy) False for True;
fork_pairs(eb, Y) none for the events at dense indices 13 and 14, seq 4; the
pair stake of the event with id 2002 and the root with id 11, at the event's
own frame, 2 for 3) were given nowhere.  The readers take the cheater lists,
the branch -> event table and the host mirror from the index at every call,
or rebuild them under lx_index::branch_gen / roll_gen, and that holds.

Measured on an MI355X: the module, 99 tests, 6.5 s in one process; the first
case (which starts the device) 1.5 s, every other case 0.13 s or less.
"""

import copy

import numpy as np
import pytest

import ancestry_model as am
import build_model as bm
import fork_evidence_model as fm
import median_time_model as mm
import progress_model as pm
import refork_dags as rd
from abft_harness import FakeLachesis
from oracle.tdag import Event
from test_gpu_ancestry import _confirm, _state
from test_gpu_fork_evidence import _all_pairs, _cheaters
from test_gpu_progress import FIELDS
from test_gpu_refork import abft_state, copies, new_gpu, new_oracle, wmap

pytestmark = pytest.mark.gpu
NAMES = list(rd.VARIANTS)
ERR_ARG = -1
READER_OPTIONS = {"default": None, "small0": {"small_max": 0}}
NO_STATS = dict(launches=0, frame_steps=0, rounds=0, fc16=0, fc_pairs=0)


@pytest.fixture(scope="module")
def lx():
    import lachesis_hip
    return lachesis_hip


# ---------------------------------------------------------------------------- the index's readers

class Readers:
    """One handle of each reader over a VecfcIndex, and the checks of one
    point of the drive against the models over ``order``."""

    def __init__(self, lx, g, sc, times):
        self.g, self.sc, self.times = g, sc, times
        self.mt = lx.MedianTimeIndex(g)
        self.anc = lx.AncestryIndex(g)
        self.fe = lx.AncestryIndex(g)                        # fork evidence: a handle of its own
        self.labels = []                                     # the model's label table, carried across the points

    def close(self):
        for h in (self.mt, self.anc, self.fe):
            h.close()

    def model(self, order):
        m = am.Model(self.sc.validators, order)
        m.label[:len(self.labels)] = self.labels[:m.n]
        return m

    def check_median_time(self, order, what):
        ids = [e.id for e in order]
        d = mm.derived_of(self.sc.validators, order, [self.times[i] for i in ids])
        rows = [d.merged(i) for i in range(len(order))]
        assert np.array_equal(self.mt.merged_times(ids), np.array([r[1] for r in rows], dtype=np.uint64)), what
        for dflt in rd.MT_DEFAULTS:
            want = np.array([d.median(r[0], r[1], dflt) for r in rows], dtype=np.uint64)
            got = self.mt.median_time(ids, dflt)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, (what, "median", dflt, ids[bad[0]], int(got[bad[0]]), int(want[bad[0]]))
        for eid in ids[-4:]:                                 # one call per event
            i = ids.index(eid)
            assert np.array_equal(self.mt.merged_times([eid])[0], rows[i][1]), (what, eid)

    def check_observes(self, m, what):
        n = m.n
        got = self.anc.observes_dense(np.repeat(np.arange(n), n), np.tile(np.arange(n), n)).reshape(n, n)
        bad = np.argwhere(got != m.observes_matrix())
        assert bad.size == 0, (what, "observes", self.g.ids[bad[0][0]], self.g.ids[bad[0][1]])

    def check_confirm(self, m, heads, labels, what):
        hs = [self.g.pos[h.id] for h in heads]
        # the labels so far are ancestor-closed, so the reference's walk and the scan agree
        twin = copy.copy(m)
        twin.label = list(m.label)
        by_scan = [sorted(g) for g in twin.confirm_all_ancestors(hs, labels)]
        got = _confirm(self.anc, m, hs, labels)              # the walk; then labels and low-water mark
        assert [sorted(int(e) for e in g) for g in got] == by_scan, what
        self.labels = list(m.label)
        return got

    def check_fork_evidence(self, m, what):
        n_pairs = _all_pairs(self.fe, m)
        lists = _cheaters(self.fe, m, list(range(m.n)))      # all heads in one call
        return n_pairs, lists


@pytest.mark.parametrize("opt", sorted(READER_OPTIONS))
@pytest.mark.parametrize("name", NAMES)
def test_index_readers_after_refork(lx, name, opt):
    sc = rd.get(name)
    V, X, Y, n, with_z, _ = rd.VARIANTS[name]
    times = rd.times_of(name)
    o, g = new_oracle(sc), new_gpu(lx, sc, READER_OPTIONS[opt])
    rs = Readers(lx, g, sc, times)
    db = {}
    k = len(sc.P)

    def add(events):
        for e in events:
            o.add(e)
        g.add_events(events)

    add(sc.P)
    o.flush()
    g.flush(db)
    rs.mt.set_times(sc.P, [times[e.id] for e in sc.P])
    add(sc.A)
    rs.mt.set_times(sc.A, [times[e.id] for e in sc.A])
    assert rs.mt.num_times() == k + len(sc.A)

    # ---- after A, on the unflushed events: X's fork is in every table
    order = sc.P + sc.A
    m = rs.model(order)
    rs.check_median_time(order, "A")
    rs.check_observes(m, "A")
    n_pairs, lists = rs.check_fork_evidence(m, "A")
    if n >= 24 or with_z:
        assert n_pairs > 0 and any(lists)
    if n >= 24:
        assert any(c == X for l in lists for c, _, _, _ in l)
    got = rs.check_confirm(m, [sc.P[k // 2], sc.A[-1]], [7, 8], "A")   # the second head is in A
    assert any(int(e) >= k for e in got[1]) and any(int(e) < k for e in got[1])
    kept, low = rs.labels[:k], min(m.low_water(), k)

    # ---- the drop
    o.drop_not_flushed()
    g.drop_not_flushed()
    assert rs.mt.num_times() == k                            # the dropped events' times are forgotten
    assert [int(l) for l in rs.anc.labels_dense()] == kept and rs.anc.low_water() == low
    assert len(rs.anc.last_confirmed_dense()) == 0
    assert len(rs.fe.last_cheaters_dense()[0]) == 0
    rs.labels = kept
    add(sc.A2)
    # the events re-added at those indices carry no label
    assert [int(l) for l in rs.anc.labels_dense()] == kept + [0] * len(sc.A2)
    rest = sc.A2 + sc.T
    rs.mt.set_times(rest, [times[e.id] for e in rest])       # T's ahead of Add
    assert rs.mt.num_times() == k + len(rest)

    def after_drop(order, what):
        m = rs.model(order)
        _state(rs.anc, m)
        rs.check_median_time(order, what)
        rs.check_observes(m, what)
        n_pairs, lists = rs.check_fork_evidence(m, what)
        assert all(c != X for l in lists for c, _, _, _ in l), what       # X is never reported
        xs, ys, _ = rs.fe.fork_pairs_dense(np.arange(m.n), np.full(m.n, X))
        assert (xs == fm.NONE).all() and (ys == fm.NONE).all(), what
        have = {e.id for e in order}
        heads = [e for e in (sc.xc, sc.ea2, sc.eb) if e.id in have] + [order[-1]]
        rs.check_confirm(m, heads, [20 + len(order) + i for i in range(len(heads))], what)
        return lists

    # ---- after drop + A2, after T
    after_drop(sc.P + sc.A2, "A2")
    add(sc.T)
    order = sc.P + rest
    lists = after_drop(order, "T")
    at = {e.id: i for i, e in enumerate(order)}
    assert Y in {c for c, _, _, _ in lists[at[sc.eb.id]]}
    ids = [e.id for e in order]

    # ---- a handle that never saw A, and one restored from the written tables
    f = new_gpu(lx, sc, READER_OPTIONS[opt])
    f.add_events(sc.P)
    f.flush()
    f.add_events(rest)
    o.flush()
    g.flush(db)
    r = lx.VecfcIndex()
    r.restore(sc.validators, db, sc.store.get)
    nn = len(ids)
    hh, xx = [i for i in ids for _ in ids], ids * nn
    hc, cc = [i for i in ids for _ in range(V)], list(range(V)) * nn
    want = dict(
        merged=rs.mt.merged_times(ids), med=[rs.mt.median_time(ids, d) for d in rd.MT_DEFAULTS],
        obs=rs.anc.observes(hh, xx),
        pairs=[p and (frozenset(p[:2]), p[2]) for p in rs.fe.fork_pairs(hc, cc)],
        lists=[[(c, frozenset((a, b)), s) for c, a, b, s in l] for l in rs.fe.cheaters(ids)])
    for h, what in ((f, "fresh"), (r, "restored")):
        hr = Readers(lx, h, sc, times)
        hr.mt.set_times(order, [times[i] for i in ids])      # by event id: the load's dense order is its own
        assert np.array_equal(hr.mt.merged_times(ids), want["merged"]), what
        for d, w in zip(rd.MT_DEFAULTS, want["med"]):
            assert np.array_equal(hr.mt.median_time(ids, d), w), (what, d)
        assert np.array_equal(hr.anc.observes(hh, xx), want["obs"]), what
        assert [p and (frozenset(p[:2]), p[2]) for p in hr.fe.fork_pairs(hc, cc)] == want["pairs"], what
        assert [[(c, frozenset((a, b)), s) for c, a, b, s in l] for l in hr.fe.cheaters(ids)] == want["lists"], what
        hr.close()
    rs.close()
    for h in (g, f, r):
        h.ix.close()


# ---------------------------------------------------------------------------- Build without Add, frame progress

FEEDINGS = ("default", "small0", "walker_then_small")


class Engines:
    """The oracle engine (a build_model.Epoch: Build then Process per event)
    and the GPU engine side by side over copies of P + A2 + T."""

    def __init__(self, sc, feeding, monkeypatch):
        from lachesis_hip import capi
        if feeding != "default":
            monkeypatch.setitem(capi.DEFAULT_OPTIONS, "small_max", 0)       # every batch on the walker path
        self.sc, self.feeding = sc, feeding
        self.ep = bm.Epoch(sc.validators, copies(rd.kept(sc)))
        self.evs = copies(rd.kept(sc))                       # the GPU engine's events
        self.t = FakeLachesis(wmap(sc), backend="gpu")
        self.lch = self.t.lch
        self.used_sp, self.has_events = set(), set()
        self.asked = []                                      # ids of the events asked as candidates
        self._model = None
        self._ncand = 0

    def close(self):
        self.lch.close()

    # feeding ---------------------------------------------------------------
    def prefix(self, n):
        """The first n events: per event, or -- walker_then_small -- as one
        batch on the walker path, after which batches of one event take the
        small path (the host mirror is read back from the device first)."""
        if self.feeding == "walker_then_small":
            consumed, err = self.t.process_batch(self.evs[:n], claimed=False)
            assert err is None and consumed == n
            assert self.path() == "walker"
            self.lch.ix.set_option("small_max", 1 << 20)     # (the library clamps it to its kSmallMaxN)
        else:
            for e in self.evs[:n]:
                self.t.build(e)
                assert self.t.process(e) is None
        self.ep.advance(n)
        assert [e.frame for e in self.evs[:n]] == [e.frame for e in self.ep.events[:n]]
        for e in self.evs[:n]:
            self._note(e)

    def path(self):
        """The path the index's last batch took: the walker path times its
        branch assignment on the device (lx_last_stats), the small path
        assigns on the host and leaves the figure 0."""
        return "walker" if self.lch.ix.last_stats()["ms_assign"] > 0 else "small"

    def _note(self, e):
        self.has_events.add(e.creator)
        if e.seq > 1:
            self.used_sp.add(e.parents[0])
        self._model = None

    def continues_tip(self, e):
        return e.creator not in self.has_events if e.seq == 1 else e.parents[0] not in self.used_sp

    def model(self):
        if self._model is None:
            self._model = pm.ProgressModel(self.ep)
        return self._model

    # candidates ------------------------------------------------------------
    def cand(self, e):
        ep = self.ep
        return ep._cand(ep.validators.idxs[e.creator], e.seq, [ep.pos(p) for p in e.parents])

    def gpu_event(self, c):
        self._ncand += 1
        return Event(("gpu-cand", self._ncand), c.event.creator, c.event.seq, 0, c.event.parents)

    def ask(self, cands, progress=True, what=""):
        """One lx_abft_build_frames call (and one progress call) for the
        candidates against the oracle's Build and progress_model; returns the
        frames."""
        ep = self.ep
        want = [ep.oracle_frame(c) for c in cands]
        evs = [self.gpu_event(c) for c in cands]
        roots = self.lch.build_frames(evs)
        assert [e.frame for e in evs] == want, what
        assert roots == [f != ep.self_parent_frame(c) for f, c in zip(want, cands)], what
        if progress:
            m = self.model()
            got = self.lch.build_progress(evs, pairs=True)
            off, root_ids, stake, total = self.lch.progress_pairs()
            assert int(off[len(cands)]) == total
            for i, c in enumerate(cands):
                F = m.frame(c)[1]
                assert F == want[i] == int(got["frame"][i]), (what, i)
                exp = m.progress(c, F)
                for k in FIELDS:
                    assert int(got[k][i]) == exp[k], (what, i, k, int(got[k][i]), exp[k])
                a, b = int(off[i]), int(off[i + 1])
                assert [(ep.pos(r), int(s)) for r, s in zip(root_ids[a:b], stake[a:b])] == exp["pairs"], (what, i)
        return want

    def step(self, i, claimed=False):
        """Event i: asked as a candidate first if it continues its branch's
        tip, then Build + Process on both engines."""
        e, eo = self.evs[i], self.ep.events[i]
        want = None
        if self.continues_tip(e):
            want = self.ask([self.cand(e)], True, ("event", e.id))[0]
            self.asked.append(e.id)
        self.ep.advance(i + 1)
        if claimed:
            e.frame = eo.frame
            consumed, err = self.t.process_batch([e], claimed=True)
            assert err is None and consumed == 1
        else:
            self.t.build(e)
            assert self.t.process(e) is None
        assert e.frame == eo.frame and (want is None or want == e.frame), e.id
        assert self.path() == ("walker" if self.feeding == "small0" else "small"), e.id
        self._note(e)

    def tips_in_one_call(self, what):
        """Every tip's candidate with 0, 1 and all other tips as parents in one
        call; the same one by one."""
        V = self.sc.V
        cands = self.ep.tip_candidates([0, 1, V - 1])
        want = self.ask(cands, True, what)
        for c, f in zip(cands, want):
            ev = self.gpu_event(c)
            self.lch.build_frames([ev])
            assert ev.frame == f, what
        return cands

    # the candidates that must be refused ------------------------------------
    def _raw(self, fn, cands, **kw):
        res = fn(self.lch.L, self.lch.h, *bm.dense(cands), **kw)
        return res[0], res[1], self.lch.L.lx_abft_last_error(self.lch.h).decode()

    def refusals(self, forks):
        """Right after the rollback, P alone processed."""
        from lachesis_hip import abft
        ep, sc = self.ep, self.sc
        n = ep.done
        assert n == len(sc.P) == self.lch.ix.num_events()
        _, last_of = ep.tips()
        xt, other = last_of[sc.X], last_of[sc.me]
        x_seq = ep.events[xt].seq + 1
        good = ep._cand(sc.X, x_seq, [xt, other])            # X goes on, on its original tip
        self.ask([good], True, "X's tip")
        stats = self.lch.last_stats()
        bad = [(ep._cand(sc.X, x_seq, [xt, n]), "parent out of range")]     # the dense index X's fork event had
        for f in forks:
            c = self.cand(f)
            assert ep.opens_branch(c)
            bad.append((c, "would open a new branch"))
        for c, text in bad:
            for at, cands in ((0, [c, good]), (1, [good, c])):
                for fn, kw in ((abft.build_frames_arrays, {}), (abft.build_progress_arrays, dict(pairs=True))):
                    rc, err, msg = self._raw(fn, cands, **kw)
                    assert (rc, err) == (ERR_ARG, at) and text in msg and "candidate %d" % at in msg, (text, at, msg)
                    assert self.lch.build_stats() == NO_STATS, text
        assert self.lch.last_stats() == stats
        return good

    # the surroundings of the read-only calls --------------------------------
    def surroundings(self, sample):
        st, ix = self.lch.state(), self.lch.ix
        ls, cr = ix.branches_info()
        return dict(n=ix.num_events(), B=ix.num_branches(), last_seq=ls.tolist(), creators=cr.tolist(),
                    epoch=st["epoch"], last=st["last_decided_frame"], ev_frame=st["ev_frame"].tobytes(),
                    ev_conf=st["ev_confirmed_on"].tobytes(), root_off=st["root_off"].tobytes(),
                    root_ev=st["root_ev"].tobytes(), hb=ix.highest_before_batch(sample),
                    la=ix.lowest_after_batch(sample), merged=ix.merged_highest_before_batch(sample),
                    branch=[ix.branch(i) for i in sample], blocks=list(self.t.block_list))

    def reads_only(self, good):
        """One build_frames and one progress call right after the rollback
        change nothing around them."""
        n = self.ep.done
        sample = sorted(set(range(n - min(n, 12), n)) | set(good.parents))
        before = self.surroundings(sample)
        assert before["n"] == n and before["B"] == self.ep.orc.num_branches()
        cands = self.ep.tip_candidates([1])
        evs = [self.gpu_event(c) for c in cands]
        self.lch.build_frames(evs)
        assert self.lch.build_stats()["launches"] > 0
        self.lch.build_progress(evs, pairs=True)
        self.lch.event_progress(self.evs[n - 3:n], pairs=True)
        assert self.surroundings(sample) == before

    # processed events --------------------------------------------------------
    def events_progress(self, what):
        """lx_abft_event_progress with pairs for every processed event at its
        own frame: the sums against progress_model, every pair stake against
        the plain count on the oracle's rows."""
        ep, m = self.ep, self.model()
        n = ep.done
        got = self.lch.event_progress(self.evs[:n], pairs=True)
        off, root_ids, stake, total = self.lch.progress_pairs()
        assert int(off[n]) == total
        assert [int(f) for f in got["frame"]] == [e.frame for e in ep.events[:n]], what
        for i in range(n):
            f = ep.events[i].frame
            exp = m.event_progress(i, f)
            for k in FIELDS:
                assert int(got[k][i]) == exp[k], (what, i, k, int(got[k][i]), exp[k])
            a, b = int(off[i]), int(off[i + 1])
            pairs = [(ep.pos(r), int(s)) for r, s in zip(root_ids[a:b], stake[a:b])]
            assert pairs == exp["pairs"], (what, i)
            rs = m.roots.get(f, [])
            plain = pm.oracle_pair_stakes(ep.orc, i, rs, m.w, m.branch_creator, m.V)
            assert [s for _, s in pairs] == [int(x) for x in plain], (what, i)

    def finish(self):
        """The whole epoch gave the oracle's frames, blocks and last decided frame."""
        ep, t = self.ep, self.t
        assert ep.done == len(self.evs)
        assert [t.lch.frame_of(e.id) for e in self.evs] == [e.frame for e in ep.events]
        want = abft_state(ep.flk)
        assert abft_state(t) == want
        assert self.sc.X + 1 not in {c for b in want["blocks"] for c in b[3]}


@pytest.mark.parametrize("feeding", FEEDINGS)
@pytest.mark.parametrize("name", NAMES)
def test_build_frames_and_progress_build_x_then_process_y(lx, name, feeding, monkeypatch):
    """The drive of test_abft_build_x_then_process_y: Build(fork of X) adds,
    evaluates and drops; the first candidates asked afterwards are A2's."""
    sc = rd.get(name, abft=True)
    k, n2 = len(sc.P), len(sc.P) + len(sc.A2)
    d = Engines(sc, feeding, monkeypatch)
    try:
        d.prefix(k)
        for f, fo in zip(copies(sc.fx), copies(sc.fx)):      # built, never processed
            d.t.build(f)
            d.ep.flk.build(fo)
            assert f.frame == fo.frame
        good = d.refusals(sc.fy)
        d.reads_only(good)
        d.tips_in_one_call("after the rollback")
        for i in range(k, len(d.evs)):
            d.step(i)
            if i + 1 == n2:
                d.events_progress("A2")
        d.events_progress("T")
        d.tips_in_one_call("T")
        fy2 = next(e for e in sc.A2 + sc.T if e.seq > 1 and e.parents[0] == sc.fy[0].id)
        assert fy2.id in d.asked and sc.fy[0].id not in d.asked    # the fork branch's second event was a candidate
        assert sc.xc.id in d.asked
        d.finish()
    finally:
        d.close()


@pytest.mark.parametrize("feeding", FEEDINGS)
@pytest.mark.parametrize("k", [0, 5])
@pytest.mark.parametrize("name", NAMES)
def test_build_frames_and_progress_after_refused_claim(lx, name, k, feeding, monkeypatch):
    """The drive of test_abft_refused_claim_then_fork_of_y: a claimed batch of
    k honest events and X's fork event with a wrong claim is refused there
    (restore + DropNotFlushed, the prefix redone).  With k = 0 the candidate
    calls are the first to evaluate a frame after the drop."""
    sc = rd.get(name, abft=True)
    n1, n2 = len(sc.P), len(sc.P) + len(sc.A2)
    d = Engines(sc, feeding, monkeypatch)
    try:
        d.prefix(n1 - k)
        tail = d.evs[n1 - k:n1]
        d.ep.advance(n1)
        fo = copies(sc.fx[:1])[0]
        d.ep.flk.build(fo)
        batch = tail + copies(sc.fx[:1])
        for e, eo in zip(batch, d.ep.events[n1 - k:n1] + [fo]):
            e.frame = eo.frame
        batch[-1].frame += 1
        consumed, err = d.t.process_batch(batch, claimed=True)
        assert consumed == k and err is not None
        for e in tail:
            d._note(e)
        good = d.refusals(sc.fy)
        d.reads_only(good)
        d.tips_in_one_call("after the refused batch")
        for i in range(n1, len(d.evs)):
            d.step(i, claimed=True)
            if i + 1 == n2:
                d.events_progress("A2")
        d.events_progress("T")
        d.tips_in_one_call("T")
        fy2 = next(e for e in sc.A2 + sc.T if e.seq > 1 and e.parents[0] == sc.fy[0].id)
        assert fy2.id in d.asked and sc.fy[0].id not in d.asked and sc.xc.id in d.asked
        d.finish()
    finally:
        d.close()
