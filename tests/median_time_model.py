"""CPU model of vecmt's merged HighestBeforeTime and MedianTime, in two forms.

*carried*  (:class:`CarriedIndex`): the restated vecfc index
  (oracle/vecfc_oracle.py) with a HighestBefore that carries a creation time
  per branch beside the seq, as the production "vecmt" index does: Init sets
  the event's own time, the join (CollectFrom) copies the parent's time exactly
  when it raises the seq, the gather (GatherFrom) copies the time of the
  winning branch, or 0 on a fork.

*derived*  (:class:`Derived`): nothing is carried.  From the C oracle's rows
  (raw HighestBefore bytes, branch ids, merged HighestBefore) and a
  (branch, seq) -> event map: a branch is a self-parent chain of consecutive
  seqs, so the highest observed seq of a branch names one event, and the time
  vecmt carries for that branch is that event's creation time.  This is what
  include/lachesis_mediantime.h computes on the device.

An entry of a merged vector is (kind, time): kind FORK (time 0), NONE
(unobserved, time 0) or SEEN.
"""

import numpy as np

from oracle import corc, tdag
from oracle import vecfc_oracle as vo

FORK, NONE, SEEN = 0, 1, 2
MASK64 = (1 << 64) - 1

# (V, events per node, parents, cheaters, forks, seed)
SHAPES = [
    (1, 6, 1, 0, 0, 1),
    (4, 6, 3, 0, 0, 2),
    (7, 25, 3, 0, 0, 1),
    (12, 30, 4, 3, 5, 2),
    (40, 12, 6, 8, 4, 3),
    (9, 20, 3, 9, 4, 7),
    (65, 4, 5, 0, 0, 4),
    (257, 3, 8, 5, 2, 6),
]
DEFAULTS = (5, 1 << 40, MASK64)


def skewed(n):
    return [max(1, 4096 // (i + 1)) for i in range(n)]


def event_times(n, seed):
    """One event in four far above 2^63, the others close together: ties, and
    values that only compare right unsigned."""
    rng = tdag.SplitMix64(seed + 100)
    out = []
    for _ in range(n):
        if rng.below(4) == 0:
            out.append((1 << 63) + rng.below(50))
        else:
            out.append(1000 + rng.below(40))
    return out


def median_time(entries, weights, default_time):
    """MedianTime over merged entries [(kind, time)] in validator idx order."""
    pairs = []
    for (kind, t), w in zip(entries, weights):
        if kind == FORK:
            pairs.append((0, 0))
        elif kind == NONE:
            pairs.append((default_time, w))
        else:
            pairs.append((t, w))
    half = sum(w for _, w in pairs) // 2
    acc = 0
    for t, w in sorted(pairs, key=lambda p: p[0]):
        acc += w
        if acc >= half:
            return t
    raise AssertionError("no pairs")


class CarriedIndex(vo.Index):
    """vecfc_oracle.Index whose HighestBefore carries a time per branch."""

    def __init__(self, time_of):
        super().__init__()
        self.time_of = time_of          # event id -> creation time
        self.vtime = {}                 # event id -> [time per branch]

    def _fill_event_vectors(self, e):
        super()._fill_event_vectors(e)
        nb = len(self.bi.creator_idxs)
        me = self.get_event_branch_id(e.id)
        seq, fork, t = [0] * nb, [False] * nb, [0] * nb
        seq[me], t[me] = e.seq, self.time_of[e.id]          # InitWithEvent
        for p in e.parents:                                  # CollectFrom, parents in order
            pv, pt = self.get_highest_before(p), self.vtime[p]
            for b in range(nb):
                his = pv.get(b)
                if his[0] == 0 and his != vo.FORK_DETECTED:
                    continue
                if fork[b]:
                    continue
                if his == vo.FORK_DETECTED:
                    fork[b] = True
                elif seq[b] < his[0]:
                    seq[b] = his[0]
                    t[b] = pt[b] if b < len(pt) else 0
        final = self.get_highest_before(e.id)
        for b in range(nb):                                  # the seqs this join tracked are the index's
            if not final.is_fork_detected(b):
                assert not fork[b] and final.seq(b) == seq[b], (e, b)
        self.vtime[e.id] = t

    def merged(self, eid):
        """[(kind, time)] per validator (GetMergedHighestBefore with times)."""
        hb, vt = self.get_highest_before(eid), self.vtime[eid]
        out = []
        for branches in self.bi.by_creators:
            best, time, kind = 0, 0, NONE
            for b in branches:
                bs = hb.get(b)
                if bs == vo.FORK_DETECTED:
                    best, time, kind = 0, 0, FORK
                    break
                if bs[0] > best:
                    best, time, kind = bs[0], vt[b], SEEN
            out.append((kind, time))
        return out


class Derived:
    """Merged times and medians from the C oracle's rows; dense indices."""

    def __init__(self, weights):
        self.w = np.array(weights, dtype=np.uint64)
        self.V = len(weights)
        self.o = corc.OracleIndex(weights)
        self.creator, self.seq, self.times = [], [], []
        self._maps = None

    def add(self, creator, seq, poff, par, times):
        assert self.o.add_batch(creator, seq, poff, par) == -1
        self.creator += list(map(int, creator))
        self.seq += list(map(int, seq))
        self.times += list(map(int, times))
        self._maps = None

    def maps(self):
        """(event of (branch, seq) as a 2-D array, branches by creator)."""
        if self._maps is None:
            n = len(self.seq)
            br = [self.o.branch(i) for i in range(n)]
            B = max(br + [self.V - 1]) + 1
            ev = np.full((B, max(self.seq + [0]) + 1), -1, dtype=np.int64)
            by = [[v] for v in range(self.V)]
            seen = set(range(self.V))
            for i in range(n):
                assert ev[br[i], self.seq[i]] == -1
                ev[br[i], self.seq[i]] = i
                if br[i] not in seen:
                    seen.add(br[i])
                    by[self.creator[i]].append(br[i])
            for l in by:
                assert l == sorted(l)
            multi = [v for v in range(self.V) if len(by[v]) > 1]
            self._maps = (ev, by, np.array(self.times + [0], dtype=np.uint64), multi)
        return self._maps

    def merged(self, i):
        """(kind[V], time[V], winning branch[V]) of event i."""
        ev, by, times, multi = self.maps()
        raw = np.frombuffer(self.o.hb(i), dtype=np.uint32).reshape(-1, 2)
        mg = np.frombuffer(self.o.merged_hb(i), dtype=np.uint32).reshape(-1, 2)
        mseq = np.zeros(self.V, dtype=np.int64)
        mmin = np.zeros(self.V, dtype=np.int64)
        k = min(self.V, len(mg))
        mseq[:k], mmin[:k] = mg[:k, 0], mg[:k, 1]
        fork = (mseq == 0) & (mmin == vo.MAX_INT32)
        kind = np.where(fork, FORK, np.where(mseq == 0, NONE, SEEN))
        win = np.arange(self.V)
        for v in multi:
            if kind[v] == SEEN:
                for b in by[v]:
                    if b < len(raw) and raw[b, 0] == mseq[v] and raw[b, 1] != vo.MAX_INT32:
                        win[v] = b
                        break
                else:
                    raise AssertionError("merged seq on no branch")
        src = np.where(kind == SEEN, ev[win, np.where(kind == SEEN, mseq, 0)], len(times) - 1)
        assert (src >= 0).all()
        return kind, np.where(kind == SEEN, times[src], np.uint64(0)), win

    def median(self, kind, time, default_time):
        t = np.where(kind == NONE, np.uint64(default_time), time).astype(np.uint64)
        w = np.where(kind == FORK, np.uint64(0), self.w)
        half = int(w.sum()) // 2
        order = np.argsort(t, kind="stable")
        k = int(np.searchsorted(np.cumsum(w[order]), half, side="left"))
        return int(t[order[k]])


def build_shape(shape, weights=None):
    """(validators, events, times by dense index) of a SHAPES entry."""
    from oracle import pos
    V, epn, P, cheaters, forks, seed = shape
    nodes, events = tdag.rand_fork_dag(V, epn, P, cheaters, forks, seed=seed)
    w = weights if weights is not None else skewed(V)
    validators = pos.Validators(dict(zip(nodes, w)))
    return validators, events, event_times(len(events), seed)


def derived_of(validators, events, times):
    d = Derived(validators.weights)
    cr, sq, off, par = tdag.to_dense(events, validators)
    d.add(cr, sq, off, par, times)
    return d
