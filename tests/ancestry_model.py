"""CPU model of include/lachesis_ancestry.h.

*walk*   : ancestor sets by one parents-first pass (a Python int per event,
  bit x = x is the event or an ancestor of it), and :meth:`Model.confirm`, the
  reference's confirmEvents (abft/lachesis.go:40-55 over abft/traversal.go:
  13-37): a stack walk from the head that labels what it reaches and stops at
  labelled events.

*rules*  : the two rules the kernels rest on, evaluated on the C oracle's rows
  (``corc.OracleIndex.la`` / ``.hb`` / ``.branch``) for all pairs at once:
    LA rule  x is a or an ancestor of a  <=>  0 < LA(x)[branch(a)] <= seq(a)
    HB rule  x is a or an ancestor of a  <=>  HB(a)[branch(x)].Seq >= seq(x),
             wherever that entry is no fork marker.

Dense indices throughout (positions in Add order).
"""

import numpy as np

from oracle import corc, pos, tdag
from oracle import vecfc_oracle as vo

# (V, events per node, parents, cheaters, forks, seed)
PAIR_SHAPES = [
    (1, 6, 1, 0, 0, 1),
    (4, 6, 3, 0, 0, 2),
    (7, 25, 3, 0, 0, 1),
    (12, 30, 4, 3, 5, 2),
    (40, 12, 6, 8, 4, 3),
    (9, 20, 3, 9, 4, 7),
    (65, 4, 5, 0, 0, 4),
    (257, 3, 8, 5, 2, 6),
    (20, 15, 4, 6, 6, 11),
    (6, 40, 3, 3, 10, 5),
]
# equal weights: (shape, blocks the oracle decides at least)
BLOCK_SHAPES = [
    ((7, 25, 3, 0, 0, 1), 11),
    ((12, 30, 4, 3, 5, 2), 7),
    ((40, 12, 6, 8, 4, 3), 3),
    ((6, 40, 3, 1, 10, 5), 11),
    ((10, 40, 4, 3, 6, 9), 11),
]


def build_shape(shape, weights=None):
    """(validators, events) of a shape; equal weights unless given."""
    V, epn, P, cheaters, forks, seed = shape
    nodes, events = tdag.rand_fork_dag(V, epn, P, cheaters, forks, seed=seed)
    w = weights if weights is not None else [1] * V
    return pos.Validators(dict(zip(nodes, w))), events


class Model:
    def __init__(self, validators, events):
        self.validators = validators
        self.n = len(events)
        self.creator, self.seq, self.poff, self.par = tdag.to_dense(events, validators)
        self.parents = [[int(p) for p in self.par[int(self.poff[i]):int(self.poff[i + 1])]] for i in range(self.n)]
        self.anc = []
        for i, ps in enumerate(self.parents):
            m = 1 << i
            for p in ps:
                assert p < i                                 # parents first
                m |= self.anc[p]
            self.anc.append(m)
        self.label = [0] * self.n
        self._rows = None

    # walk ------------------------------------------------------------------
    def observes(self, head, x):
        return bool((self.anc[head] >> x) & 1)

    def observes_matrix(self):
        """[head, x] for all pairs."""
        out = np.zeros((self.n, self.n), dtype=bool)
        for a in range(self.n):
            bits = bin(self.anc[a])[:1:-1]
            out[a, :len(bits)] = np.frombuffer(bits.encode(), dtype=np.uint8) == ord("1")
        return out

    def confirm(self, heads, labels):
        """Per head, in call order, the events it labelled (DFS order)."""
        out = []
        for head, lab in zip(heads, labels):
            assert lab != 0
            got, stack = [], [int(head)]
            while stack:
                e = stack.pop()
                if self.label[e] != 0:
                    continue
                self.label[e] = int(lab)
                got.append(e)
                stack.extend(self.parents[e])
            out.append(got)
        return out

    def confirm_all_ancestors(self, heads, labels):
        """What lx_anc_confirm does after arbitrary labels: every unlabelled
        ancestor, also behind a labelled event."""
        out = []
        for head, lab in zip(heads, labels):
            got = [e for e in range(int(head) + 1) if (self.anc[head] >> e) & 1 and self.label[e] == 0]
            for e in got:
                self.label[e] = int(lab)
            out.append(got)
        return out

    def low_water(self):
        return next((i for i, l in enumerate(self.label) if l == 0), self.n)

    # rules -----------------------------------------------------------------
    def rows(self):
        """(oracle, branch[n], hb seq [n, B], hb marked [n, B], la [n, B])."""
        if self._rows is None:
            o = corc.OracleIndex(self.validators.weights)
            assert o.add_batch(self.creator, self.seq, self.poff, self.par) == -1
            B = o.num_branches()
            branch = np.array([o.branch(i) for i in range(self.n)], dtype=np.int64)
            hb_seq = np.zeros((self.n, B), dtype=np.int64)
            hb_mark = np.zeros((self.n, B), dtype=bool)
            la = np.zeros((self.n, B), dtype=np.int64)
            for i in range(self.n):
                r = np.frombuffer(o.hb(i), dtype=np.uint32).reshape(-1, 2)
                mark = (r[:, 0] == 0) & (r[:, 1] == vo.MAX_INT32)
                hb_seq[i, :len(r)] = np.where(mark, 0, r[:, 0])
                hb_mark[i, :len(r)] = mark
                l = np.frombuffer(o.la(i), dtype=np.uint32)
                la[i, :len(l)] = l
            self._rows = (o, branch, hb_seq, hb_mark, la)
        return self._rows

    def la_rule_matrix(self):
        """[head, x]: 0 < LA(x)[branch(head)] <= seq(head)."""
        _, branch, _, _, la = self.rows()
        l = la[:, branch].T                                  # [head, x] = la[x, branch[head]]
        sq = np.asarray(self.seq, dtype=np.int64)[:, None]
        return (l > 0) & (l <= sq)

    def hb_rule_matrix(self):
        """([head, x] HB(head)[branch(x)].Seq >= seq(x), [head, x] entry is a fork marker)."""
        _, branch, hb_seq, hb_mark, _ = self.rows()
        sq = np.asarray(self.seq, dtype=np.int64)[None, :]
        return hb_seq[:, branch] >= sq, hb_mark[:, branch]


def oracle_blocks(validators, events):
    """The blocks corc.AbftOracle decides on the DAG in one batch:
    [(frame, atropos, cheaters (creator idx), confirmed events)]."""
    cr, sq, off, par = tdag.to_dense(events, validators)
    o = corc.AbftOracle(validators.weights)
    rc, consumed, _ = o.process_batch(cr, sq, off, par)
    assert rc == 0 and consumed == len(events)
    return [(b[1], b[2], b[3], b[4]) for b in o.blocks]
