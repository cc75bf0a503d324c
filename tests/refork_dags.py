"""Rollback, then a fork by another creator (tests/test_refork_dags.py,
tests/test_gpu_refork.py, tests/test_gpu_refork_readers.py).

A fork gives its creator the next branch number (vecengine/index.go:105-141),
DropNotFlushed takes it back (vecengine/index.go:88-96), and the next fork --
possibly of another creator -- gets the same number: the branch count returns
to a value it had before with another branch -> creator map behind it.  Every
table built from that map and kept across calls has to notice.

A scenario (``Scenario``) is a flushed prefix ``P``, a batch ``A`` with a fork
event of creator X (two of them in the "two" variant), a batch ``A2`` of the
same length with a fork event of Y != X (and of W) in which X stays honest, and
a tail ``T`` added after ``A2`` (the rest of the same continuation; with
``len(A) == 1``, the per-event cadence, all of it).  The continuation of A2
holds, by construction:

* ``fy``  Y's fork event: a second child of ``Y_prev``, so it takes the number
  X's fork event had in ``A``; ``fy2`` continues that branch and observes xc;
* ``xc``  (c) an event of X that (a) and (b) observe;
* ``ea``  (a) one parent on Y's fork branch and nothing of Y's original branch
  beyond ``Y_prev`` (Y's last event of P, ``Y_head``, is observed by nobody in
  P): merged HighestBefore[Y] comes from the fork column;
* ``eb``  (b) observes ``Y_head`` and the fork branch: fork marker at Y;
* ``ea2`` on top of ``ea``, ``fy2`` and one event of each helper creator, each
  of which observes xc: ForklessCause(ea2, xc) counts X, (a)'s creator, the
  helpers and Y -- Y through the fork column alone -- which is exactly the
  quorum of equal weights (3 of 4, 4 of 5, 6 of 8).  Without Y's fork branch
  the answer is False; with the fork column credited to X (the map of ``A``)
  X is counted twice and the answer is False too;

and then seeded random rounds whose events see either of Y's branches.  ``A``
is the same construction with X and Y swapped, so every consumer has tables
of X's fork to go stale.

``reshuffled`` is the epoch of a ``rand_fork_dag`` with several cheaters that
is rolled back to the last flush at random points and redone in another
parents-first order, so that other creators fork first.

Seeded with SplitMix64; plain Python, importable without a GPU.
"""

from oracle import pos, tdag
from oracle import vecfc_oracle as vo
from oracle.tdag import Event, SplitMix64
from abft_harness import topo_shuffle

P_ROUNDS = 3


def shard_split(V, G=2):
    """First creator idx of shard 1 of 2 (lx_shard_range: V * q / G, rounded
    down to a multiple of 4)."""
    return (V * 1 // G) & ~3


class _Builder:
    """Events over creator idxs 0..V-1 (validator id = idx + 1, equal weights:
    idx order = id order)."""

    def __init__(self, V, rng):
        self.V, self.rng = V, rng
        self.main = [[] for _ in range(V)]     # each creator's original-branch events
        self.by_id = {}

    def mk(self, eid, c, sp, others, line=None):
        parents = ([sp.id] if sp is not None else []) + [o.id for o in others if sp is None or o.id != sp.id]
        lam = 1 + max([self.by_id[p].lamport for p in parents], default=0)
        e = Event(eid, c + 1, sp.seq + 1 if sp is not None else 1, lam, parents, "e%d" % eid)
        self.by_id[eid] = e
        if line is not None:
            line.append(e)
        return e

    def head(self, c):
        return self.main[c][-1]

    def pick(self, c, k, heads):
        """k distinct creators other than c that have a head in ``heads``."""
        cand = [o for o in range(self.V) if o != c and heads.get(o) is not None]
        out = []
        while cand and len(out) < k:
            out.append(cand.pop(self.rng.below(len(cand))))
        return out


class Scenario:
    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def validators(self):
        return pos.Validators({c + 1: 1 for c in range(self.V)})

    @property
    def store(self):
        return {e.id: e for e in self.P + self.A + self.A2 + self.T}

    def without_fork(self):
        """A2 + T without Y's (and W's) fork branches: the fork events and
        their self-descendants removed, and taken out of every parent list."""
        gone = set(self.fork_branch_ids)
        out = []
        for e in self.A2 + self.T:
            if e.id in gone:
                continue
            c = Event(e.id, e.creator, e.seq, e.lamport, [p for p in e.parents if p not in gone], e.name)
            out.append(c)
        return out


def _continuation(b, eid, F, C, Ea, Eb, helpers, G, n_total):
    """The events after P in which F forks (G: the creator of a second fork
    or None) and C stays honest; returns (events, roles)."""
    rng, V = b.rng, b.V
    out = []
    nxt = [eid]

    def mk(c, sp, others, line=None):
        e = b.mk(nxt[0], c, sp, others, line)
        nxt[0] += 1
        out.append(e)
        return e

    main = [list(l) for l in b.main]          # this continuation's own view of the original branches
    F_head, F_prev = main[F][-1], main[F][-2]
    fy = mk(F, F_prev, [main[Ea][-1]])
    fork_line = [fy]
    forks = [fy]
    if G is not None:
        forks.append(mk(G, main[G][-2], [main[Eb if Eb != G else Ea][-1]]))
    xc = mk(C, main[C][-1], [main[Eb][-1]], main[C])
    hs = [mk(h, main[h][-1], [xc], main[h]) for h in helpers]
    fy2 = mk(F, fy, [xc], fork_line)
    ea = mk(Ea, main[Ea][-1], [fy, xc], main[Ea])
    ea2 = mk(Ea, ea, [fy2] + hs, main[Ea])
    eb = mk(Eb, main[Eb][-1], [F_head, fy2, xc], main[Eb])
    quorum = V * 2 // 3 + 1
    while len(out) < n_total:
        c = rng.below(V)
        heads = {o: main[o][-1] for o in range(V)}
        if rng.below(2):
            heads[F] = fork_line[-1]
        others = [heads[o] for o in b.pick(c, quorum - 1, heads)]
        if c == F and rng.below(2):
            mk(F, fork_line[-1], others, fork_line)
        else:
            mk(c, main[c][-1], others, main[c])
    roles = dict(fork=fy, forks=forks, xc=xc, ea=ea, ea2=ea2, eb=eb, fy2=fy2, F_head=F_head,
                 fork_branch_ids=[e.id for e in fork_line] + [f.id for f in forks[1:]])
    return out, roles


def _roles(V, X, Y):
    rest = [c for c in range(V) if c not in (X, Y)]
    quorum = V * 2 // 3 + 1
    Ea, Eb = rest[0], rest[1]
    helpers = rest[2:2 + quorum - 3]
    assert len(helpers) == quorum - 3
    return Ea, Eb, helpers


def scenario(V, X, Y, n, with_z=False, two=False, seed=1):
    """One re-fork scenario; see the module docstring.  ``n`` = len(A) =
    len(A2) (>= 2 with ``two``); ``with_z``: P holds the fork of an older
    cheater Z (the creator of (b)), so B_flushed = V + 1; ``two``: A holds two
    fork events of X, A2 one of Y and one of W (the creator of (b))."""
    assert X != Y and not (with_z and two) and n >= (2 if two else 1)
    rng = SplitMix64(seed * 1000003 + V * 101 + X * 17 + Y * 5 + n)
    b = _Builder(V, rng)
    Ea, Eb, helpers = _roles(V, X, Y)
    P = []
    eid = [0]

    def mkp(c, sp, others, line):
        e = b.mk(eid[0], c, sp, others, line)
        eid[0] += 1
        P.append(e)
        return e

    for r in range(P_ROUNDS):
        order = tdag.shuffle(list(range(V)), rng)
        for c in order:
            heads = {o: (b.main[o][-1] if b.main[o] else None) for o in range(V)}
            mkp(c, heads[c], [heads[o] for o in b.pick(c, 2, heads)], b.main[c])
    Z = None
    if with_z:
        Z = Eb
        fz = mkp(Z, b.main[Z][-2], [b.head(Ea)], None)
        for c in tdag.shuffle(list(range(V)), rng):
            heads = {o: b.head(o) for o in range(V)}
            others = [heads[o] for o in b.pick(c, 2, heads)]
            if c != Z:
                others.append(fz)
            mkp(c, heads[c], others, b.main[c])
    # the last events of X and Y: observed by nobody in P
    ends = {}
    for c in (X, Y):
        heads = {o: b.head(o) for o in range(V) if o not in ends}
        ends[c] = mkp(c, b.head(c), [heads[o] for o in b.pick(c, 1, heads)], b.main[c]).id
    total = n + max(0, 9 + len(helpers) + 3 * V - n) if n < 12 else n + 4
    W = Eb if two else None
    A_all, ra = _continuation(b, 1000, X, Y, Ea, Eb, helpers, X if two else None, n)
    S, rs = _continuation(b, 2000, Y, X, Ea, Eb, helpers, W, total)
    return Scenario(V=V, X=X, Y=Y, Z=Z, W=W, n=n, me=Ea, P=P, A=A_all[:n], A2=S[:n], T=S[n:], seed=seed,
                    fx=ra["forks"], fy=rs["forks"], xc=rs["xc"], ea=rs["ea"], ea2=rs["ea2"], eb=rs["eb"],
                    fork_branch_ids=rs["fork_branch_ids"], with_z=with_z, two=two)


def drive_oracle(sc, second="A2"):
    """vecfc_oracle.Index after P, flush, A, DropNotFlushed, A2, T; returns
    (index, branch ids X's fork events had in A)."""
    rest = sc.A2 + sc.T if second == "A2" else sc.without_fork()
    store = sc.store
    store.update({e.id: e for e in rest})
    o = vo.Index()
    o.reset(sc.validators, store.get)
    for e in sc.P:
        o.add(e)
    o.flush()
    for e in sc.A:
        o.add(e)
    bx = [o.get_event_branch_id(f.id) for f in sc.fx]
    o.drop_not_flushed()
    for e in rest:
        o.add(e)
    return o, bx


def stale_forkless_cause(o, sc, a_id, b_id, bx):
    """ForklessCause(a, b) of vecfc/forkless_cause.go:28-82 with the fork
    columns ``bx`` credited to X, as tables built for ``A`` have them."""
    creators = list(o.bi.creator_idxs)
    for br in bx:
        creators[br] = sc.X
    a, b = o.get_highest_before(a_id), o.get_lowest_after(b_id)
    seen, total = set(), 0
    for branch, creator in enumerate(creators):
        la, hb = b.get(branch), a.get(branch)
        if la <= hb[0] and la != 0 and tuple(hb) != vo.FORK_DETECTED and creator not in seen:
            seen.add(creator)
            total += 1
    return total >= sc.validators.quorum()


def frames_of(sc, events):
    """Frames of P + events from abft_harness.FakeLachesis (Build + Process
    per event)."""
    from abft_harness import FakeLachesis
    t = FakeLachesis({c + 1: 1 for c in range(sc.V)})
    out = {}
    for e in sc.P + events:
        c = Event(e.id, e.creator, e.seq, e.lamport, e.parents, e.name)
        t.build(c)
        assert t.process(c) is None
        out[e.id] = c.frame
    return out


def discriminates(sc, abft=False):
    """None when the scenario meets every condition of
    tests/test_refork_dags.py, else the name of the first one it misses."""
    o, bx = drive_oracle(sc)
    if [o.get_event_branch_id(f.id) for f in sc.fy] != bx:
        return "branch ids"
    m = o.get_merged_highest_before(sc.ea.id)
    if not m.get(sc.Y)[0] > o.get_highest_before(sc.ea.id).get(sc.Y)[0]:
        return "(a)"
    m = o.get_merged_highest_before(sc.eb.id)
    if not (m.is_fork_detected(sc.Y) and not m.is_fork_detected(sc.X)):
        return "(b)"
    for e in (sc.ea, sc.eb):
        if o.get_highest_before(e.id).get(sc.X)[0] < sc.xc.seq:
            return "(c)"
    o0, _ = drive_oracle(sc, "nofork")
    if not (o.forkless_cause(sc.ea2.id, sc.xc.id) and not o0.forkless_cause(sc.ea2.id, sc.xc.id)):
        return "quorum edge"
    if stale_forkless_cause(o, sc, sc.ea2.id, sc.xc.id, bx):
        return "stale map"
    if abft:
        f1, f0 = frames_of(sc, sc.A2 + sc.T), frames_of(sc, sc.without_fork())
        if not any(f1[k] != f0[k] for k in f0):
            return "frames"
    return None


def found(V, X, Y, n, with_z=False, two=False, abft=False, seed=1):
    """The first scenario from ``seed`` on that discriminates."""
    for s in range(seed, seed + 64):
        sc = scenario(V, X, Y, n, with_z, two, s)
        if discriminates(sc, abft) is None:
            return sc
    raise AssertionError("no discriminating scenario for %r" % ((V, X, Y, n, with_z, two, abft),))


# name: V, X, Y, len(A), P holds cheater Z, two forks change owner
VARIANTS = {
    "v4_y_below": (4, 2, 0, 1, False, False),        # idx(Y) < idx(X), the per-event cadence
    "v4_y_above": (4, 0, 3, 24, False, False),
    "v5_z": (5, 1, 3, 1, True, False),               # B_flushed = V + 1
    "v5_z_long": (5, 4, 0, 30, True, False),
    "v8_split_lo_hi": (8, 1, 6, 1, False, False),    # X in shard 0, Y in shard 1 of 2
    "v8_split_hi_lo": (8, 5, 2, 36, False, False),
    "v8_split_z": (8, 2, 7, 1, True, False),
    "v5_two": (5, 0, 2, 2, False, True),             # two numbers change owner
    "v8_two_long": (8, 6, 1, 28, False, True),
}

_cache = {}


def get(name, abft=False):
    key = (name, abft)
    if key not in _cache:
        _cache[key] = found(*VARIANTS[name], abft=abft)
    return _cache[key]


# ---------------------------------------------------------------------------- per reader
#
# One condition per reader of the branch tables that tests/test_gpu_refork_readers.py
# drives: some query's right answer differs from the answer computed with the
# fork columns of ``A`` still credited to X (``stale_map``), or with the first
# seq X's fork branch had.  Each function returns the differing queries; an
# empty list means that a stale table could pass in that scenario.

MT_DEFAULTS = (0, 1 << 40)


def kept(sc):
    """The events present after drop + A2 + T, in Add order."""
    return sc.P + sc.A2 + sc.T


def stale_map(o, sc, bx):
    """(creator_idxs, by_creators) of the oracle with the branch numbers ``bx``
    credited to X, as tables built for ``A`` have them."""
    creators = list(o.bi.creator_idxs)
    for br in bx:
        creators[br] = sc.X
    by = [[] for _ in range(sc.V)]
    for b, c in enumerate(creators):
        by[c].append(b)
    return creators, by


def event_times(sc, seed):
    """{event id: creation time} for P, A, A2 and T: mostly close together, one
    in five far above 2^63; the events of A and of A2 at the same dense index
    get different times."""
    rng = SplitMix64(seed * 7919 + sc.V * 131 + sc.n)
    out = {}
    for e in sc.P + sc.A + sc.A2 + sc.T:
        out[e.id] = (1 << 63) + rng.below(97) if rng.below(5) == 0 else 1000 + rng.below(400)
    return out


def drive_carried(sc, times):
    """median_time_model.CarriedIndex through P, flush, A, drop, A2, T."""
    import median_time_model as mm
    o = mm.CarriedIndex(times)
    o.reset(sc.validators, sc.store.get)
    for e in sc.P:
        o.add(e)
    o.flush()
    for e in sc.A:
        o.add(e)
    bx = [o.get_event_branch_id(f.id) for f in sc.fx]
    o.drop_not_flushed()
    for e in kept(sc)[len(sc.P):]:
        o.add(e)
    return o, bx


def merged_times_by_map(o, eid, by_creators):
    """CarriedIndex.merged over an explicit creator -> branches map."""
    import median_time_model as mm
    hb, vt = o.get_highest_before(eid), o.vtime[eid]
    out = []
    for branches in by_creators:
        best, time, kind = 0, 0, mm.NONE
        for b in branches:
            bs = tuple(hb.get(b))
            if bs == vo.FORK_DETECTED:
                best, time, kind = 0, 0, mm.FORK
                break
            if bs[0] > best:
                best, time, kind = bs[0], vt[b] if b < len(vt) else 0, mm.SEEN
        out.append((kind, time))
    return out


def median_time_diffs(sc, times):
    """[(head id, default, right median, stale median)] over the heads ea and
    eb and MT_DEFAULTS where the two medians differ."""
    import median_time_model as mm
    o, bx = drive_carried(sc, times)
    _, stale_by = stale_map(o, sc, bx)
    w = sc.validators.weights
    out = []
    for head in (sc.ea, sc.eb):
        right = merged_times_by_map(o, head.id, o.bi.by_creators)
        assert right == o.merged(head.id)
        stale = merged_times_by_map(o, head.id, stale_by)
        for dflt in MT_DEFAULTS:
            a, b = mm.median_time(right, w, dflt), mm.median_time(stale, w, dflt)
            if a != b:
                out.append((head.id, dflt, a, b))
    return out


_times = {}


def times_of(name):
    """The scenario's creation times: the first seed under which the medians
    at ea and at eb both differ under the stale map (None if none of 64
    does)."""
    if name not in _times:
        sc = get(name)
        _times[name] = None
        for seed in range(1, 65):
            t = event_times(sc, seed)
            heads = {d[0] for d in median_time_diffs(sc, t)}
            if heads == {sc.ea.id, sc.eb.id}:
                _times[name] = t
                break
    return _times[name]


def observes_by_map(o, creators, head, x):
    """x is head or an ancestor of it, from the oracle's rows (the rule of
    lx_anc_observes): HighestBefore(head)[branch(x)].Seq >= seq(x), and where
    head has detected the fork of the branch's creator -- marks are per
    creator: the entry of the creator's original branch tells -- the
    LowestAfter rule.  ``head`` is x or comes after it in Add order."""
    if head.id == x.id:
        return True
    hb = o.get_highest_before(head.id)
    b = o.get_event_branch_id(x.id)
    if hb.is_fork_detected(creators[b]):
        la = o.get_lowest_after(x.id).get(o.get_event_branch_id(head.id))
        return 0 < la <= head.seq
    ent = tuple(hb.get(b))
    return ent != vo.FORK_DETECTED and ent[0] >= x.seq


def ancestry_diffs(sc):
    """[(head id, x id)] where the stale map changes observes(head, x); asserts
    that the right map gives the ancestor sets of the parent lists."""
    import ancestry_model as am
    o, bx = drive_oracle(sc)
    stale, _ = stale_map(o, sc, bx)
    order = kept(sc)
    m = am.Model(sc.validators, order)
    out = []
    for i, head in enumerate(order):
        for j in range(i + 1):
            right = observes_by_map(o, o.bi.creator_idxs, head, order[j])
            assert right == m.observes(i, j), (head.id, order[j].id)
            if observes_by_map(o, stale, head, order[j]) != right:
                out.append((head.id, order[j].id))
    return out


def fork_evidence_diffs(sc):
    """([(head id, creator, right, stale)], same with X's first seq): the
    branch-interval rule of lx_anc_fork_pairs over the stale creator -> branches
    map, and over the right map with the reused numbers' first seq taken from
    X's fork branches; asserts that the right tables give the naive answer."""
    import ancestry_model as am
    import fork_evidence_model as fm
    o, bx = drive_oracle(sc)
    order = kept(sc)
    m = am.Model(sc.validators, order)
    br = fm.Branches(m)
    cnt = fm.observed_counts(m, br)
    marked = m.rows()[3]                                     # [head, branch]: the entry is a fork marker
    right_of = {c: list(l) for c, l in br.of_creator.items()}
    stale_of = {c: [b for b in l if b not in bx] for c, l in right_of.items()}
    stale_of[sc.X] = sorted(stale_of.get(sc.X, []) + list(bx))
    right_first = list(br.first)
    stale_first = list(br.first)
    for b, f in zip(bx, sc.fx):
        stale_first[b] = f.seq
    by_map, by_first = [], []
    for h in range(len(sc.P), m.n):
        naive = fm.evidence_row(m, h)
        for c in range(sc.V):
            br.of_creator, br.first = right_of, right_first
            right = fm.interval_rule(br, cnt[h], c)
            assert right == naive.get(c, fm.NO_EVIDENCE), (order[h].id, c)
            if not marked[h, c]:                             # no fork of c detected: nothing is looked up
                assert right == fm.NO_EVIDENCE
                continue
            br.of_creator = stale_of
            stale = fm.interval_rule(br, cnt[h], c)
            if stale != right:
                by_map.append((order[h].id, c, right, stale))
            br.of_creator, br.first = right_of, stale_first
            try:
                stale = fm.interval_rule(br, cnt[h], c)
            except IndexError:                               # the pair's place lies outside the branch
                stale = None
            if stale != right:
                by_first.append((order[h].id, c, right, stale))
    br.of_creator, br.first = right_of, right_first
    return by_map, by_first


def cheaters_seen(sc, events, heads):
    """{head id: set of creators} by the naive rule over ``events``."""
    import ancestry_model as am
    import fork_evidence_model as fm
    m = am.Model(sc.validators, events)
    at = {e.id: i for i, e in enumerate(events)}
    return {h.id: set(fm.evidence_row(m, at[h.id])) for h in heads}


def progress_epoch(sc):
    """build_model.Epoch over P + A2 + T, all processed (Build of X's fork
    event in between, as tests/test_gpu_refork.py drives it)."""
    import build_model as bm
    evs = [Event(e.id, e.creator, e.seq, e.lamport, e.parents, e.name) for e in kept(sc)]
    ep = bm.Epoch(sc.validators, evs)
    ep.advance(len(sc.P))
    for f in sc.fx:
        ep.flk.build(Event(f.id, f.creator, f.seq, f.lamport, f.parents, f.name))
    ep.advance(len(evs))
    return ep


def progress_diffs(sc):
    """[(event id, root id, right stake, stale stake)]: the pair stakes of
    every processed event at its own frame (lx_abft_event_progress), counted
    with the fork columns credited to X."""
    import progress_model as pm
    _, bx = drive_oracle(sc)
    ep = progress_epoch(sc)
    m = pm.ProgressModel(ep)
    right = {e: m.event_pair_stakes(e, m.roots.get(int(m.frames[e]), [])) for e in range(m.n)}
    for b in bx:
        assert m.branch_creator[b] != sc.X
        m.branch_creator[b] = sc.X
    m._finish()
    out = []
    for e in range(m.n):
        rs = m.roots.get(int(m.frames[e]), [])
        for r, a, b in zip(rs, right[e], m.event_pair_stakes(e, rs)):
            if a != b:
                out.append((ep.events[e].id, ep.events[r].id, int(a), int(b)))
    return out


READERS = ("median_time", "ancestry", "fork_evidence", "progress")
_reader_diffs = {}


def reader_diffs(name):
    """{reader: differing queries} of a variant (the abft readers on the
    ``abft`` scenario of that name), computed once."""
    if name not in _reader_diffs:
        sc = get(name)
        t = times_of(name)
        _reader_diffs[name] = {
            "median_time": median_time_diffs(sc, t) if t is not None else [],
            "ancestry": ancestry_diffs(sc),
            "fork_evidence": fork_evidence_diffs(sc)[0],
            "progress": progress_diffs(get(name, abft=True)),
        }
    return _reader_diffs[name]


# ---------------------------------------------------------------------------- reshuffled redo

RESHUFFLE_SHAPE = (8, 16, 4, 5, 12)      # nodes, events/node, parents, cheaters, forks


def reshuffled_ops(seed):
    """(validators, store, ops): ops = ("add", events) | ("flush",) |
    ("drop",) over the events of a rand_fork_dag; after every drop the events
    behind the last flush are redone in another parents-first order."""
    V, epn, pc, ch, fk = RESHUFFLE_SHAPE
    rng = SplitMix64(seed)
    nodes, evs = tdag.rand_fork_dag(V, epn, pc, cheaters=ch, forks_count=fk, rng=rng)
    validators = pos.Validators({v: 1 + k % 3 for k, v in enumerate(nodes)})
    order = list(evs)
    ops = []
    i = i_flushed = drops = 0
    must_flush = False
    redo = 0
    while i < len(order):
        part = order[i:i + max(redo, 1 + rng.below(8))]     # a redo covers at least what was dropped
        redo = 0
        ops.append(("add", part))
        i += len(part)
        r = rng.below(100)
        if not must_flush and r < 50 and drops < 40:
            ops.append(("drop",))
            order[i_flushed:] = topo_shuffle(order[i_flushed:], rng)
            redo = i - i_flushed
            i = i_flushed
            drops += 1
            must_flush = True
        elif must_flush or r < 75 or i >= len(order):
            ops.append(("flush",))
            i_flushed = i
            must_flush = False
    return validators, {e.id: e for e in evs}, ops


def owner_changes(validators, store, ops):
    """Rollbacks after which a branch number the dropped events had created
    belongs to another creator once the events are redone."""
    o = vo.Index()
    o.reset(validators, store.get)
    o.init_branches_info()
    changed = 0
    before = None
    flushed_B = len(validators)
    for op in ops:
        if op[0] == "add":
            for e in op[1]:
                o.add(e)
            if before is not None:
                now = o.bi.creator_idxs
                if any(b < len(now) and now[b] != c for b, c in before.items()):
                    changed += 1
                before = None
        elif op[0] == "flush":
            o.flush()
            flushed_B = len(o.bi.creator_idxs)
        else:
            before = {b: c for b, c in enumerate(o.bi.creator_idxs) if b >= flushed_B}
            o.drop_not_flushed()
    return changed


_reshuffled = {}


def reshuffled(min_changes=3, seed=1):
    if "r" not in _reshuffled:
        for s in range(seed, seed + 64):
            validators, store, ops = reshuffled_ops(s)
            if owner_changes(validators, store, ops) >= min_changes:
                _reshuffled["r"] = (validators, store, ops)
                break
        else:
            raise AssertionError("no reshuffled epoch with %d owner changes" % min_changes)
    return _reshuffled["r"]
