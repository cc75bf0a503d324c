"""CPU model of lx_abft_build_frames (include/lachesis_abft.h):
the frame of a candidate event that is NOT added, from the rows the index
already holds.

*rows*   : the C oracle's HighestBefore / LowestAfter rows of every event of
  the epoch so far (``corc.OracleIndex`` getters), as numpy planes.
*rule*   : the candidate's virtual HighestBefore row (join of the parents'
  rows, own entry, the two fork rules of vecengine/index.go:173-209 with
  MinSeq = the branch's first seq), ForklessCause on that row and the roots'
  LowestAfter rows with the own-branch column replaced by "r is a parent of e
  or an ancestor of one", and calcFrameIdx's loop over the oracle engine's
  root lists.
*epoch*  : :class:`Epoch` drives ``oracle.abft_oracle.IndexedLachesis`` (Build
  then Process per event) and forms the candidates the tests ask about.

Dense indices throughout (positions in Add order).
"""

import numpy as np

import abft_harness as ah
from oracle import tdag
from oracle import vecfc_oracle as vo

BUILD_CAP = 100          # calcFrameIdx: selfParentFrame + 100 in Build

# (V, events per node, parents, cheaters, forks, seed)
FORK_FREE_SHAPES = [(1, 6, 1, 0, 0, 1), (3, 12, 3, 0, 0, 2), (16, 40, 5, 0, 0, 1)]
FORK_SHAPES = [(12, 30, 4, 3, 5, 2), (24, 30, 6, 5, 6, 2)]
SHAPES = FORK_FREE_SHAPES + FORK_SHAPES


class Cand:
    """A candidate event: dense fields for the C ABI / the model and the
    tdag.Event the oracle's Build takes."""

    __slots__ = ("creator", "seq", "parents", "event", "tip", "k")

    def __init__(self, creator, seq, parents, event, tip=None, k=None):
        self.creator, self.seq, self.parents, self.event, self.tip, self.k = creator, seq, parents, event, tip, k


def dense(cands):
    """(creator, seq, parent_off, parent_idx) of a candidate list."""
    cr = np.array([c.creator for c in cands], dtype=np.uint32)
    sq = np.array([c.seq for c in cands], dtype=np.uint32)
    off = np.zeros(len(cands) + 1, dtype=np.uint64)
    flat = []
    for i, c in enumerate(cands):
        flat.extend(c.parents)
        off[i + 1] = len(flat)
    return cr, sq, off, np.array(flat if flat else [0], dtype=np.uint32)


class Epoch:
    """One epoch on the oracle engine, event by event (Build, then Process)."""

    def __init__(self, validators, events):
        self.validators = validators
        self.events = list(events)
        self.flk = ah.FakeLachesis(dict(zip(validators.ids, validators.weights)))
        self.done = 0
        self._ncand = 0

    @classmethod
    def of_shape(cls, shape, weights=None):
        from oracle import pos
        V, epn, P, cheaters, forks, seed = shape
        nodes, events = tdag.rand_fork_dag(V, epn, P, cheaters, forks, seed=seed)
        w = weights if weights is not None else [1] * V
        return cls(pos.Validators(dict(zip(nodes, w))), events)

    def advance(self, upto):
        """Process events [done, upto); returns them."""
        out = self.events[self.done:upto]
        for e in out:
            self.flk.build(e)
            assert self.flk.process(e) is None
        self.done = max(self.done, upto)
        return out

    # the oracle's view -----------------------------------------------------
    @property
    def orc(self):
        return self.flk.index.o

    def pos(self, eid):
        return self.flk.index.pos[eid]

    def oracle_frame(self, cand):
        """IndexedLachesis.build(e): the yardstick."""
        self.flk.build(cand.event)
        return cand.event.frame

    def opens_branch(self, cand):
        """Ground truth of the branch-opening refusal: Add on the C oracle,
        look at the branch count, drop."""
        o = self.orc
        b0 = o.num_branches()
        assert o.add(cand.creator, cand.seq, cand.parents) == 0
        grew = o.num_branches() > b0
        o.drop_not_flushed()
        return grew

    def self_parent_frame(self, cand):
        if cand.seq <= 1 or not cand.parents:
            return 0
        return self.events[cand.parents[0]].frame

    # candidates ------------------------------------------------------------
    def _cand(self, creator, seq, parents, tip=None, k=None):
        self._ncand += 1
        ids = [self.events[p].id for p in parents]
        ev = tdag.Event(("cand", self._ncand), self.validators.ids[creator], seq, 0, ids)
        return Cand(creator, seq, list(parents), ev, tip, k)

    def tips(self):
        """(branch tips: branch -> last event, last event of each validator)."""
        o = self.orc
        by_branch, last_of = {}, {}
        for i in range(self.done):
            by_branch[o.branch(i)] = i          # Add order: a branch is a chain
            last_of[self.validators.idxs[self.events[i].creator]] = i
        return by_branch, last_of

    def tip_candidates(self, ks):
        """For every branch tip and every k of ks: parents = the tip plus the
        last events of k other validators (the next ones in idx order that
        have events)."""
        by_branch, last_of = self.tips()
        V = len(self.validators)
        out = []
        for b in sorted(by_branch):
            t = by_branch[b]
            c = self.validators.idxs[self.events[t].creator]
            others = [last_of[(c + d) % V] for d in range(1, V) if (c + d) % V in last_of]
            for k in ks:
                out.append(self._cand(c, self.events[t].seq + 1, [t] + others[:min(k, len(others))], t, k))
        return out

    def off_tip_candidates(self):
        """Candidates the call refuses: a self-parent that is not its
        branch's last event, and seq 1 for a creator that has events."""
        by_branch, last_of = self.tips()
        tips = set(by_branch.values())
        out = []
        for i in range(self.done):
            if i in tips or len(out) >= 8:
                continue
            c = self.validators.idxs[self.events[i].creator]
            out.append(self._cand(c, self.events[i].seq + 1, [i]))
        for c, t in sorted(last_of.items())[:2]:
            others = [x for v, x in sorted(last_of.items()) if v != c][:2]
            out.append(self._cand(c, 1, others))
        return out


class Model:
    """The rule over the oracle's rows at one point of an :class:`Epoch`."""

    def __init__(self, ep):
        self.ep = ep
        o, n = ep.orc, ep.done
        self.n = n
        self.B = B = o.num_branches()
        self.V = len(ep.validators)
        self.w = np.array(ep.validators.weights, dtype=np.int64)
        self.quorum = ep.validators.quorum()
        self.creator = np.array([ep.validators.idxs[e.creator] for e in ep.events[:n]], dtype=np.int64)
        self.seq = np.array([e.seq for e in ep.events[:n]], dtype=np.int64)
        self.branch = np.array([o.branch(i) for i in range(n)], dtype=np.int64)
        self.hb_seq = np.zeros((n, B), dtype=np.int64)
        self.hb_mark = np.zeros((n, B), dtype=bool)
        self.la = np.zeros((n, B), dtype=np.int64)
        for i in range(n):
            r = np.frombuffer(o.hb(i), dtype=np.uint32).reshape(-1, 2)
            mark = (r[:, 0] == 0) & (r[:, 1] == vo.MAX_INT32)
            self.hb_seq[i, :len(r)] = np.where(mark, 0, r[:, 0])
            self.hb_mark[i, :len(r)] = mark
            l = np.frombuffer(o.la(i), dtype=np.uint32)
            self.la[i, :len(l)] = l
        # BranchesInfo: creator, first and last seq per branch
        self.branch_creator = np.full(B, -1, dtype=np.int64)
        self.branch_creator[:self.V] = np.arange(self.V)
        self.branch_first = np.zeros(B, dtype=np.int64)
        self.branch_last = np.zeros(B, dtype=np.int64)
        for i in range(n):
            b = self.branch[i]
            self.branch_creator[b] = self.creator[i]
            if self.branch_first[b] == 0:
                self.branch_first[b] = self.seq[i]
            self.branch_last[b] = self.seq[i]
        self.by_creator = [[b for b in range(B) if self.branch_creator[b] == c] for c in range(self.V)]
        # the engine's root slots, in its order
        self.roots = {}
        f = 1
        while ep.flk.store.get_frame_roots(f):
            self.roots[f] = [ep.pos(r.id) for r in ep.flk.store.get_frame_roots(f)]
            f += 1

    # the documented LX_ERR_ARG rules ---------------------------------------
    def refusal(self, c):
        """None, or why lx_abft_build_frames refuses the candidate."""
        if c.creator >= self.V:
            return "creator"
        if c.seq == 0:
            return "seq"
        if any(p >= self.n for p in c.parents):
            return "parent"
        if len(set(c.parents)) != len(c.parents):
            return "duplicate"
        own_first = bool(c.parents) and self.creator[c.parents[0]] == c.creator
        if c.seq == 1:
            if own_first:
                return "self-parent"
            return "branch" if self.branch_last[c.creator] else None
        if not own_first or self.seq[c.parents[0]] != c.seq - 1:
            return "self-parent"
        if self.branch_last[self.branch[c.parents[0]]] != c.seq - 1:
            return "branch"
        return None

    # 1. the virtual HighestBefore row --------------------------------------
    def own_branch(self, c):
        return int(self.branch[c.parents[0]]) if c.seq > 1 else c.creator

    def virtual_row(self, c):
        """(seq[B], marked[B], marked by the parents' rows alone [B])."""
        be = self.own_branch(c)
        s = np.zeros(self.B, dtype=np.int64)
        m = np.zeros(self.B, dtype=bool)
        for p in c.parents:                                   # CollectFrom: max, the marker absorbing
            s = np.maximum(s, self.hb_seq[p])
            m |= self.hb_mark[p]
        if not m[be]:
            s[be] = c.seq                                     # InitWithEvent; the parents' entries are below
        s[m] = 0
        inherited = m.copy()
        for n in range(self.V):
            brs = self.by_creator[n]
            if len(brs) < 2:
                continue
            hit = bool(m[brs].any())                          # (i) one marked branch marks all
            if not hit:                                       # (ii) overlapping [first seq, seq]
                live = [b for b in brs if s[b] != 0]
                first = {b: (self.branch_first[b] if self.branch_first[b] else c.seq) for b in live}
                hit = any(first[x] <= s[y] and first[y] <= s[x] for x in live for y in live if x != y)
            if hit:
                m[brs] = True
                s[brs] = 0
        return s, m, inherited

    # 2. ForklessCause(e, r) -------------------------------------------------
    def is_ancestor(self, c, r):
        """r is a parent of e or an ancestor of one."""
        return any(p == r or 0 < self.la[r, self.branch[p]] <= self.seq[p] for p in c.parents)

    def forkless_cause(self, c, row, r, corrected=True):
        s, m, _ = row
        if m[self.branch[r]]:                                 # forkless_cause.go:49-54
            return False
        la = self.la[r]
        term = (la != 0) & (la <= s) & ~m
        if corrected:
            be = self.own_branch(c)
            term[be] = (not m[be]) and self.is_ancestor(c, r)
        yes = np.zeros(self.V, dtype=bool)
        yes[self.branch_creator[np.nonzero(term)[0]]] = True   # a creator counts once across its branches
        return int(self.w[yes].sum()) >= self.quorum

    # 3. the frame loop ------------------------------------------------------
    def quorum_on(self, c, row, f, corrected=True):
        yes = np.zeros(self.V, dtype=bool)
        for r in self.roots.get(f, []):
            if self.forkless_cause(c, row, r, corrected):
                yes[self.creator[r]] = True
        return int(self.w[yes].sum()) >= self.quorum

    def frame(self, c, corrected=True):
        """(selfParentFrame, frame) as calcFrameIdx with checkOnly = false."""
        spf = self.ep.self_parent_frame(c)
        row = self.virtual_row(c)
        f = spf
        while f < spf + BUILD_CAP and self.quorum_on(c, row, f, corrected):
            f += 1
        return spf, max(f, 1)
