"""CPU model of lx_abft_build_progress / lx_abft_event_progress
(include/lachesis_abft.h) on top of tests/build_model.py: the
stake behind ForklessCause(e, r) and what a frame's root slots add up to.

*pair stake*  : 0 if HB(e)[branch(r)] is a fork marker, otherwise the weight of
  the distinct creators with a branch j where 0 < LA(r)[j] <= HB(e)[j].Seq --
  the WeightCounter of forklessCause before HasQuorum.  For a candidate that
  is not added: the virtual row and the corrected own-branch column of
  build_model; for an indexed event: the oracle's rows as they are.
*per frame*   : over the engine's root slots of f in its order, the slot of e
  itself left out: n_caused (stake >= quorum), stake (weight of the distinct
  creators of those slots), root_stake (sum of min(stake, quorum)).

:class:`ProgressModel` is built from a ``build_model.Epoch`` (the Python
engine) or, :meth:`ProgressModel.from_ref`, from a ``build_cases.Ref`` (the C
restatement the GPU tests drive).
"""

import numpy as np

import build_model as bm
from oracle import vecfc_oracle as vo


def planes(o, n, B):
    """HighestBefore (seq, marked) and LowestAfter of events [0, n) of the C oracle."""
    hb_seq = np.zeros((n, B), dtype=np.int64)
    hb_mark = np.zeros((n, B), dtype=bool)
    la = np.zeros((n, B), dtype=np.int64)
    for i in range(n):
        r = np.frombuffer(o.hb(i), dtype=np.uint32).reshape(-1, 2)
        mark = (r[:, 0] == 0) & (r[:, 1] == vo.MAX_INT32)
        hb_seq[i, :len(r)] = np.where(mark, 0, r[:, 0])
        hb_mark[i, :len(r)] = mark
        l = np.frombuffer(o.la(i), dtype=np.uint32)
        la[i, :len(l)] = l
    return hb_seq, hb_mark, la


class ProgressModel(bm.Model):
    def __init__(self, ep):
        super().__init__(ep)
        self.frames = np.array([e.frame for e in ep.events[:self.n]], dtype=np.int64)
        self._finish()

    @classmethod
    def from_ref(cls, ref, roots):
        """The model over a build_cases.Ref after ``ref.advance``; roots =
        {frame: [root events in slot order]}."""
        m = cls.__new__(cls)
        d, o, n = ref.d, ref.orc, ref.done
        m.ep = None
        m.n = n
        m.B = B = o.num_branches()
        m.V = d.V
        m.w = np.array(d.weights, dtype=np.int64)
        m.quorum = ref.quorum
        m.creator = d.creator[:n].astype(np.int64)
        m.seq = d.seq[:n].astype(np.int64)
        m.branch = np.array([o.branch(i) for i in range(n)], dtype=np.int64)
        m.hb_seq, m.hb_mark, m.la = planes(o, n, B)
        m.branch_creator = np.full(B, -1, dtype=np.int64)
        m.branch_creator[:m.V] = np.arange(m.V)
        m.branch_first = np.zeros(B, dtype=np.int64)
        m.branch_last = np.zeros(B, dtype=np.int64)
        for i in range(n):
            b = m.branch[i]
            m.branch_creator[b] = m.creator[i]
            if m.branch_first[b] == 0:
                m.branch_first[b] = m.seq[i]
            m.branch_last[b] = m.seq[i]
        m.by_creator = [[] for _ in range(m.V)]
        for b in range(B):
            m.by_creator[m.branch_creator[b]].append(b)
        m.roots = {int(f): [int(r) for r in rs] for f, rs in roots.items() if len(rs)}
        m.frames = ref.frames[:n].astype(np.int64)
        m._finish()
        return m

    def _finish(self):
        self.onehot = None
        if self.B > self.V:
            self.onehot = np.zeros((self.B, self.V), dtype=np.float32)
            self.onehot[np.arange(self.B), self.branch_creator] = 1

    def self_parent_frame(self, c):
        if c.seq <= 1 or not c.parents:
            return 0
        return int(self.frames[c.parents[0]])

    def build_frame(self, c):
        """(selfParentFrame, Build frame) without the Python engine."""
        spf = self.self_parent_frame(c)
        row = self.virtual_row(c)
        f = spf
        while f < spf + bm.BUILD_CAP and self.progress(c, f, row)["stake"] >= self.quorum:
            f += 1
        return spf, max(f, 1)

    # pair stakes -------------------------------------------------------------
    def _count(self, term, s_mark, rs):
        """stake per root from the per-branch terms (R x B)."""
        if self.onehot is None:
            yes = term
        else:
            yes = (term.astype(np.float32) @ self.onehot) > 0     # a creator counts once across its branches
        stake = yes.astype(np.int64) @ self.w
        stake[s_mark[self.branch[rs]]] = 0                        # forkless_cause.go:49-54
        return stake

    def pair_stakes(self, c, row, rs, corrected=True):
        """stake(e, r) of candidate c (virtual row ``row``) for the roots rs."""
        s, m, _ = row
        rs = np.asarray(rs, dtype=np.int64)
        if not len(rs):
            return np.zeros(0, dtype=np.int64)
        la = self.la[rs]
        term = (la != 0) & (la <= s[None, :]) & ~m[None, :]
        if corrected:
            be = self.own_branch(c)
            ps = np.asarray(c.parents, dtype=np.int64)
            anc = np.zeros(len(rs), dtype=bool)
            if len(ps):
                lp = la[:, self.branch[ps]]
                anc = ((rs[:, None] == ps[None, :]) | ((lp != 0) & (lp <= self.seq[ps][None, :]))).any(axis=1)
            term[:, be] = anc & (not m[be])
        return self._count(term, m, rs)

    def event_pair_stakes(self, e, rs):
        """stake(e, r) of indexed event e: the oracle's rows as they are."""
        rs = np.asarray(rs, dtype=np.int64)
        if not len(rs):
            return np.zeros(0, dtype=np.int64)
        s, m = self.hb_seq[e], self.hb_mark[e]
        la = self.la[rs]
        return self._count((la != 0) & (la <= s[None, :]) & ~m[None, :], m, rs)

    # per frame ----------------------------------------------------------------
    def _sums(self, rs, stakes, own):
        rs = np.asarray(rs, dtype=np.int64)
        keep = rs != own if len(rs) else np.zeros(0, dtype=bool)
        caused = (stakes >= self.quorum) & keep
        yes = np.zeros(self.V, dtype=bool)
        yes[self.creator[rs[caused]]] = True
        return dict(n_roots=len(rs), n_caused=int(caused.sum()), stake=int(self.w[yes].sum()),
                    root_stake=int(np.minimum(stakes, self.quorum)[keep].sum()),
                    pairs=[(int(r), int(x)) for r, x in zip(rs, stakes)])

    def progress(self, c, f, row=None, corrected=True):
        """Candidate c at frame f."""
        rs = self.roots.get(f, [])
        row = self.virtual_row(c) if row is None else row
        return self._sums(rs, self.pair_stakes(c, row, rs, corrected), -1)

    def event_progress(self, e, f):
        """Indexed event e at frame f; its own slot is left out of the sums."""
        rs = self.roots.get(f, [])
        return self._sums(rs, self.event_pair_stakes(e, rs), e)


def oracle_pair_stakes(o, e, rs, weights, branch_creator, V):
    """Plain forklessCause counting on the C oracle's rows as they stand now:
    stake(e, r) for event e (e.g. a candidate just added) and the roots rs."""
    B = o.num_branches()
    r = np.frombuffer(o.hb(e), dtype=np.uint32).reshape(-1, 2)
    m = np.zeros(B, dtype=bool)
    s = np.zeros(B, dtype=np.int64)
    mark = (r[:, 0] == 0) & (r[:, 1] == vo.MAX_INT32)
    m[:len(r)] = mark
    s[:len(r)] = np.where(mark, 0, r[:, 0])
    w = np.asarray(weights, dtype=np.int64)
    out = []
    for root in rs:
        if m[o.branch(root)]:
            out.append(0)
            continue
        la = np.zeros(B, dtype=np.int64)
        l = np.frombuffer(o.la(root), dtype=np.uint32)
        la[:len(l)] = l
        term = (la != 0) & (la <= s) & ~m
        yes = np.zeros(V, dtype=bool)
        yes[branch_creator[np.nonzero(term)[0]]] = True
        out.append(int(w[yes].sum()))
    return np.array(out, dtype=np.int64)
