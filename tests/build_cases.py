"""Dense-index cases for the GPU tests of lx_abft_build_frames
(tests/test_gpu_build_frames.py): DAGs as arrays, the C abft restatement
(``corc.AbftOracle``: Process per event, ``abo_build`` = IndexedLachesis.Build
of one event) as the yardstick, and the candidates the tests ask about.

Importable without a GPU: tests/test_build_cases.py asserts from the oracle
alone that the cases are what the GPU tests need."""

import ctypes

import numpy as np

from oracle import corc, tdag


class Dense:
    """Events of one epoch as the C ABI takes them."""

    def __init__(self, weights, creator, seq, poff, par):
        self.weights = [int(w) for w in weights]
        self.creator = np.ascontiguousarray(creator, dtype=np.uint32)
        self.seq = np.ascontiguousarray(seq, dtype=np.uint32)
        self.poff = np.ascontiguousarray(poff, dtype=np.uint64)
        self.par = np.ascontiguousarray(par, dtype=np.uint32)

    def __len__(self):
        return len(self.creator)

    @property
    def V(self):
        return len(self.weights)

    def slice(self, lo, hi):
        a, b = int(self.poff[lo]), int(self.poff[hi])
        return self.creator[lo:hi], self.seq[lo:hi], self.poff[lo:hi + 1] - self.poff[lo], self.par[a:b]

    def parents(self, i):
        return [int(p) for p in self.par[int(self.poff[i]):int(self.poff[i + 1])]]


def shape_dag(shape, weights=None):
    """gen_dag(n, ev, p, cheaters, forks, seed) as a :class:`Dense`; weights in
    idx order (default: equal, so idx order = node order)."""
    V, epn, P, cheaters, forks, seed = shape
    nodes, events = tdag.rand_fork_dag(V, epn, P, cheaters, forks, seed=seed)
    w = list(weights) if weights is not None else [1] * V

    class _V:                                               # idx = generation column, whatever the weights
        idxs = {n: i for i, n in enumerate(nodes)}
    return Dense(w, *tdag.to_dense(events, _V))


def star_dag(V, rounds=3):
    """Width case: three heavy validators (idx 0, V // 2, V - 1: the first, a
    middle and the last column) hold the quorum; every event's parents are its
    self-parent and the heavy validators' latest events, so quorums form
    through columns at both ends of the row and frames advance within three
    events per validator."""
    heavy = sorted({0, V // 2, V - 1})
    w = [1] * V
    for h in heavy:
        w[h] = 1000
    creator, seq, poff, par = [], [], [0], []
    last = [-1] * V
    order = heavy + [c for c in range(V) if c not in heavy]  # heavy roots first: the oracle's quorum loops stop early
    for k in range(rounds):
        for c in order:
            ps = ([last[c]] if last[c] >= 0 else []) + [last[h] for h in heavy if h != c and last[h] >= 0]
            creator.append(c)
            seq.append(k + 1)
            par.extend(ps)
            poff.append(len(par))
            last[c] = len(creator) - 1
    return Dense(w, creator, seq, poff, par)


def silent_dag(rounds):
    """Many frames: four equal validators; validator 0 emits its first event
    and goes silent, the others emit one event per round on their self-parent
    and the latest events of the other two (and of validator 0)."""
    creator, seq, poff, par = [0], [1], [0, 0], []
    last = [0, -1, -1, -1]
    for k in range(rounds):
        for c in (1, 2, 3):
            ps = ([last[c]] if last[c] >= 0 else []) + [last[o] for o in (1, 2, 3, 0) if o != c and last[o] >= 0]
            creator.append(c)
            seq.append(k + 1)
            par.extend(ps)
            poff.append(len(par))
            last[c] = len(creator) - 1
    return Dense([1, 1, 1, 1], creator, seq, poff, par)


class Cand:
    __slots__ = ("creator", "seq", "parents")

    def __init__(self, creator, seq, parents):
        self.creator, self.seq, self.parents = int(creator), int(seq), [int(p) for p in parents]


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


class Ref:
    """The oracle fed the first ``upto`` events of a DAG.  Default: the C abft
    restatement (Process per event, elections included).  ``light``: frames and
    root lists by calcFrameIdx (event_processing.go:148-189) over the C index
    oracle's ForklessCause alone -- no elections, whose cost at V = 1030 (10 s
    on the CPU) the frames do not depend on; tests/test_build_cases.py holds
    the two modes equal on the narrower cases."""

    def __init__(self, d, light=False):
        self.d = d
        self.light = light
        self.abo = None if light else corc.AbftOracle(d.weights)
        self.orc = corc.OracleIndex(d.weights)               # branch ids of the events; light: ForklessCause
        self.frames = np.zeros(len(d), dtype=np.uint32)
        self.roots = {}                                      # light: frame -> root events, in order
        self.quorum = sum(d.weights) * 2 // 3 + 1
        self._w = np.array(d.weights, dtype=np.int64)
        self.done = 0

    def _calc_frame(self, e, spf):
        f = spf
        while f < spf + 100:
            roots = self.roots.get(f, [])
            if not roots:
                break
            r = np.array(roots, dtype=np.uint32)
            fc = self.orc.forkless_cause_batch_mt(np.full(len(r), e, dtype=np.uint32), r, 8).astype(bool)
            yes = np.unique(self.d.creator[r[fc]])           # a validator counts once
            if int(self._w[yes].sum()) < self.quorum:
                break
            f += 1
        return max(f, 1)

    def advance(self, upto):
        lo, hi = self.done, int(upto)
        if hi <= lo:
            return
        if not self.light:
            c, s, off, par = self.d.slice(lo, hi)
            rc, consumed, out = self.abo.process_batch(c, s, off, par)
            assert rc == 0 and consumed == hi - lo
            self.frames[lo:hi] = out
        for i in range(lo, hi):
            ps = self.d.parents(i)
            assert self.orc.add(int(self.d.creator[i]), int(self.d.seq[i]), ps) == 0
            if self.light:
                spf = int(self.frames[ps[0]]) if self.d.seq[i] > 1 and ps else 0
                f = self._calc_frame(i, spf)
                self.frames[i] = f
                for g in range(spf + 1, f + 1):
                    self.roots.setdefault(g, []).append(i)
        self.orc.flush()
        self.done = hi

    def build(self, c):
        """IndexedLachesis.Build of one candidate on the oracle."""
        if self.light:
            assert self.orc.add(c.creator, c.seq, c.parents) == 0
            try:
                return self._calc_frame(self.done, self.self_parent_frame(c))
            finally:
                self.orc.drop_not_flushed()
        p = np.ascontiguousarray(c.parents if c.parents else [0], dtype=np.uint32)
        out = ctypes.c_uint32()
        rc = self.abo.L.abo_build(self.abo.h, c.creator, c.seq, len(c.parents),
                                  p.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), ctypes.byref(out))
        assert rc == 0, rc
        return out.value

    def self_parent_frame(self, c):
        return int(self.frames[c.parents[0]]) if c.seq > 1 and c.parents else 0

    def tips(self):
        """(branch -> its last event, validator -> its last event)."""
        by_branch, last_of = {}, {}
        for i in range(self.done):
            by_branch[self.orc.branch(i)] = i
            last_of[int(self.d.creator[i])] = i
        return by_branch, last_of

    def tip_candidates(self, ks, only=None):
        """For every branch tip (``only``: these creators' tips) and every k of
        ks: parents = the tip plus the last events of the next k validators in
        idx order that have events."""
        by_branch, last_of = self.tips()
        V = self.d.V
        out = []
        for b in sorted(by_branch):
            t = by_branch[b]
            c = int(self.d.creator[t])
            if only is not None and c not in only:
                continue
            others = [last_of[(c + x) % V] for x in range(1, V) if (c + x) % V in last_of]
            for k in ks:
                out.append(Cand(c, int(self.d.seq[t]) + 1, [t] + others[:min(k, len(others))]))
        return out

    def answers(self, cands):
        """(frames, is_root) of the oracle's Build per candidate."""
        f = np.array([self.build(c) for c in cands], dtype=np.uint32)
        r = np.array([int(x) != self.self_parent_frame(c) for x, c in zip(f, cands)], dtype=np.uint8)
        return f, r


def checkpoints(n):
    """early, middle, last"""
    return sorted({max(1, n // 5), max(1, n // 2), n})


def ks_of(shape):
    return sorted({0, 1, max(shape[2] - 1, 0), shape[0] - 1})
