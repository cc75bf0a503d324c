"""Directed inputs for the stake-weighted selection kernels -- MedianTime
(k_mt<E>, lx_mediantime.hip) and the QuorumIndexer's weighted medians and
metric (k_qi_median, k_qi_metric, lx_emitter.hip) -- with numpy models of
both.  No GPU here: tests/test_selection_cases.py pins the models to the
pure-Python ones and checks that every generator reaches its edge;
tests/test_gpu_selection_edges.py feeds the same cases to the kernels.

Everything a case controls is under the caller's control in production too:
creation times per event, weights per epoch, the events processed.
"""

import numpy as np

from oracle import corc
from oracle import vecfc_oracle as vo

import median_time_model as mm
from median_time_model import FORK, NONE, SEEN

MASK64 = (1 << 64) - 1
FORK_SEQ = 0x7FFFFFFE                   # seqOf(fork detected), quorum_indexer.go:70-75
FAN = 11                                # roots a chain event takes in beside its self-parent
DEFAULT_TIMES = (0, 5, 1 << 40, MASK64)
LADDER_STEPS = (-1, 0, 1)               # weight of the low group, relative to half
METRIC_CAPS = (0, 2, 0xFFFFFFFF)
BATCHES = (1, 16, 17)                   # around kQiInline = 16; then all that is left


# ----------------------------------------------------------------------------
# DAGs as dense arrays

class Dag:
    """creator, seq, poff, par (the arguments of add_batch) and what the cases
    need to know of the events."""

    def __init__(self, V):
        self.V = V
        self.creator, self.seq, self.poff, self.par = [], [], [0], []

    def add(self, creator, seq, parents):
        self.creator.append(creator)
        self.seq.append(seq)
        self.par.extend(parents)
        self.poff.append(len(self.par))
        return len(self.creator) - 1

    def arrays(self):
        return (np.array(self.creator, dtype=np.uint32), np.array(self.seq, dtype=np.uint32),
                np.array(self.poff, dtype=np.uint64), np.array(self.par, dtype=np.uint32))

    def __len__(self):
        return len(self.creator)


def comb_dag(V, hub=0, second_layer=False):
    """One root per validator (event v is validator v's root); validator `hub`
    emits the chain c_1..c_K, c_j on its self-parent and the next <= FAN roots
    not yet included (<= 12 parents), so c_K observes everyone, c_j a prefix of
    `others` (the validators but hub, in order), a root only itself.  With
    `second_layer` every other validator v emits a seq-2 event on
    [root_v, c_j(v)], j(v) spread over 1..K."""
    d = Dag(V)
    for v in range(V):
        d.add(v, 1, [])
    d.hub = hub
    d.others = [v for v in range(V) if v != hub]
    d.K = max(1, -(-(V - 1) // FAN))
    d.chain = []                                    # chain[j - 1] = c_j
    for j in range(1, d.K + 1):
        prev = d.chain[-1] if d.chain else hub
        d.chain.append(d.add(hub, j + 1, [prev] + d.others[FAN * (j - 1):FAN * j]))
    d.j_of, d.layer2 = {}, {}
    if second_layer:
        for k, v in enumerate(d.others):
            j = 1 + (k * 7) % d.K
            d.j_of[v] = j
            d.layer2[v] = d.add(v, 2, [v, d.chain[j - 1]])
    return d


def comb_row(d, ev):
    """Merged HighestBefore seqs of a comb event, in closed form."""
    row = np.zeros(d.V, dtype=np.int64)
    c, s = d.creator[ev], d.seq[ev]
    if c == d.hub:
        j = s - 1                                   # the root is c_0
    elif s == 2:
        j = d.j_of[c]
    else:
        j = 0
    if j:
        row[d.others[:FAN * j]] = 1
        row[d.hub] = j + 1
    row[c] = s
    return row


FORK3_WEIGHTS = [1, 5, 5]


def fork3_dag():
    """Validators 1 and 2 fork at seq 2; event `narrow` of validator 0 sees one
    side of each, its child `wide` both: two fork-detected entries, honest
    weight 1."""
    d = Dag(3)
    for v in range(3):
        d.add(v, 1, [])
    a1, b1 = d.add(1, 2, [1]), d.add(1, 2, [1])
    a2, b2 = d.add(2, 2, [2]), d.add(2, 2, [2])
    d.sides = (a1, a2)
    d.narrow = d.add(0, 2, [0, a1, a2])
    d.wide = d.add(0, 3, [d.narrow, b1, b2])
    return d


# ----------------------------------------------------------------------------
# weights

def mixed_weights(V):
    """A quarter of the validators (every fourth index) skewed, the others 1;
    no weight above the number of 1s, so a greedy subset reaches every sum up
    to the total.  Total < 2^31."""
    n_big = max(1, V // 4) if V > 1 else 0
    ones = V - n_big
    w = [1] * V
    for i in range(n_big):
        w[4 * i] = max(2, min(ones, 4096) // (i + 1))
    return w


def dominant_weights(V):
    return [1 << 30] + [1] * (V - 1)


def heavy_weights(V, big=0):
    """Total exactly 2^31 - 1, all but V - 1 of it on validator `big`."""
    w = [1] * V
    w[big] = (1 << 31) - 1 - (V - 1)
    return w


def quorum_of(w):
    return (sum(w) * 2 // 3 + 1) & 0xFFFFFFFF


def subset_with_sum(w, target, order):
    """Greedy over `order`, the weights above 1 first and then the 1s: the
    members whose weights add up to `target` exactly; raises when the sweeps do
    not get there."""
    left, out = target, []
    order = list(order)
    for big in (True, False):
        for v in order:
            if (w[v] > 1) == big and left and w[v] <= left:
                out.append(v)
                left -= w[v]
    if left or sum(w[v] for v in out) != target:
        raise AssertionError("no subset of weight %d (short by %d)" % (target, left))
    return out


def placed_order(cands, where):
    """`cands` from the start, from the end, or from the middle outwards."""
    if where == "start":
        return list(cands)
    if where == "end":
        return list(cands)[::-1]
    m = len(cands) // 2
    out = []
    for k in range(len(cands)):
        i = m + (k + 1) // 2 * (1 if k % 2 else -1)
        out.append(cands[i % len(cands)])
    assert sorted(out) == sorted(cands)
    return out


# ----------------------------------------------------------------------------
# MedianTime

def np_median(kind, time, w, default_time):
    """MedianTime over merged entries as arrays (Derived.median with the
    weights as an argument)."""
    t = np.where(kind == NONE, np.uint64(default_time), time).astype(np.uint64)
    ww = np.where(kind == FORK, 0, np.asarray(w)).astype(np.int64)
    half = int(ww.sum()) // 2
    order = np.argsort(t, kind="stable")
    k = int(np.searchsorted(np.cumsum(ww[order]), half, side="left"))
    return int(t[order[k]])


class MtModel:
    """The derived model over one DAG whose times are written per case."""

    def __init__(self, w, arrays):
        self.w = list(map(int, w))
        self.V = len(w)
        self.n = len(arrays[0])
        self.d = mm.Derived(self.w)
        self.d.add(*arrays, times=range(1, self.n + 1))     # time - 1 names the source event

    def query(self, ev):
        return MtQuery(self, ev)


class MtQuery:
    """One queried event: kind per validator, the event that supplies each
    observed validator's time, and the honest weight."""

    def __init__(self, model, ev):
        self.m, self.ev = model, ev
        kind, time, _ = model.d.merged(ev)
        self.kind = np.asarray(kind)
        self.obs = np.flatnonzero(self.kind == SEEN)                 # O, validator indices
        self.src = (time[self.obs] - np.uint64(1)).astype(np.int64)  # their source events
        assert len(set(self.src.tolist())) == len(self.src)
        self.honest = sum(model.w[v] for v in np.flatnonzero(self.kind != FORK))
        self.half = self.honest // 2

    def event_times(self, t_obs):
        """Times of all events: i + 1, the sources overwritten."""
        t = np.arange(1, self.m.n + 1, dtype=np.uint64)
        t[self.src] = np.asarray(t_obs, dtype=np.uint64)
        return t

    def merged_row(self, t_obs):
        row = np.zeros(self.m.V, dtype=np.uint64)
        row[self.obs] = np.asarray(t_obs, dtype=np.uint64)
        return row

    def median(self, t_obs, default_time):
        return np_median(self.kind, self.merged_row(t_obs), self.m.w, default_time)


class MtCase:
    """Times over the observed set of a query, a default time, and the answer
    where the construction gives it (else None: the model's is taken)."""

    def __init__(self, name, t_obs, default_time=5, expect=None, **info):
        self.name, self.t, self.default, self.expect, self.info = name, t_obs, default_time, expect, info

    def __repr__(self):
        return "MtCase(%s)" % self.name


def _u64(rng, n=None):
    return rng.integers(0, 1 << 64, size=n, dtype=np.uint64)


def ladder_cases(q, seed=1):
    """For every bit b two values that first differ at b (random common prefix
    above, random lower bits equal within each group); the low group weighs
    half - 1, half, half + 1.  Needs every validator observed and half >= 1."""
    w, V = q.m.w, q.m.V
    assert len(q.obs) == V and q.half >= 1
    rng = np.random.default_rng(seed)
    order = sorted(range(V), key=lambda v: -w[v])
    n_big = sum(1 for v in order if w[v] > 1)
    out = []
    for b in range(64):
        ones = rng.permutation(order[n_big:]).tolist()         # the low group's 1s land in every slot
        for step in LADDER_STEPS:
            target = q.half + step
            low = subset_with_sum(w, target, order[:n_big] + ones)
            prefix = int(_u64(rng)) >> (b + 1) << (b + 1) if b < 63 else 0
            lo_v = prefix | (int(_u64(rng)) & ((1 << b) - 1))
            hi_v = prefix | (1 << b) | (int(_u64(rng)) & ((1 << b) - 1))
            t = np.full(V, hi_v, dtype=np.uint64)
            t[low] = lo_v
            out.append(MtCase("ladder-b%d%+d" % (b, step), t, expect=hi_v if step < 0 else lo_v,
                              bit=b, step=step, target=target, low=low, lo=lo_v, hi=hi_v))
    return out


def spread_cases(q, seed=2):
    """Random, windowed, equal and extreme times: every class that makes sense
    on any query, observed or not."""
    n = len(q.obs)
    rng = np.random.default_rng(seed + q.ev)
    out = []
    for s in range(4):
        out.append(MtCase("uniform-%d" % s, _u64(rng, n), default_time=int(_u64(rng))))
    for k in (1, 8, 33):
        x = (0b101 << 61) | (int(_u64(rng)) >> 3)              # high bits set, X + 2^k < 2^64
        t = np.uint64(x) + rng.integers(0, 1 << k, size=n, dtype=np.uint64)
        out.append(MtCase("window-k%d" % k, t, default_time=x + (1 << k) // 2, x=x, k=k))
    e = int(_u64(rng)) >> 2 | 1 << 61
    out.append(MtCase("equal", np.full(n, e, dtype=np.uint64), default_time=e,
                      expect=e if q.half and (q.kind != FORK).all() else None))
    for name, other in (("equal-but-one-below", e - 3), ("equal-but-one-above", e + 3)):
        t = np.full(n, e, dtype=np.uint64)
        t[int(rng.integers(n))] = other
        out.append(MtCase(name, t, default_time=e))
    for dflt in DEFAULT_TIMES:
        t = _u64(rng, n)
        t[rng.integers(0, n, size=max(1, n // 3))] = 0
        t[rng.integers(0, n, size=max(1, n // 3))] = MASK64
        out.append(MtCase("extremes-default%d" % dflt, t, default_time=dflt))
    out.append(MtCase("all-zero", np.zeros(n, dtype=np.uint64), default_time=MASK64))
    out.append(MtCase("all-max", np.full(n, MASK64, dtype=np.uint64), default_time=0))
    return out


def dominant_cases(q, seed=3):
    """dominant_weights: validator 0 outweighs the rest together, so its time
    is the answer wherever it stands among the others."""
    assert q.m.w[0] > sum(q.m.w[1:]) and q.obs[0] == 0 and len(q.obs) == q.m.V
    rng = np.random.default_rng(seed)
    out = []
    for name in ("smallest", "largest", "middle"):
        t = _u64(rng, q.m.V) >> np.uint64(1) | np.uint64(1 << 20)
        t[0] = {"smallest": 7, "largest": MASK64 - 7, "middle": int(np.sort(t[1:])[(q.m.V - 1) // 2])}[name]
        out.append(MtCase("dominant-" + name, t, expect=int(t[0])))
    return out


# ----------------------------------------------------------------------------
# QuorumIndexer

class QiModel:
    """emitter/ancestor.QuorumIndexer in numpy over the C oracle's merged rows.
    The matrix is kept transposed, as on the device: mt[creator][validator]."""

    def __init__(self, w, o, creator):
        self.w = np.array(w, dtype=np.int64)
        self.V = len(w)
        self.o, self.creator = o, creator
        self.quorum = quorum_of(w)
        self.reset()

    def reset(self):
        self.mt = np.zeros((self.V, self.V), dtype=np.uint32)
        self.sp = np.zeros(self.V, dtype=np.uint32)

    def seqs(self, ev):
        """seqOf of the merged row: a fork reads FORK_SEQ."""
        r = np.frombuffer(self.o.merged_hb(int(ev)), dtype=np.uint32).reshape(-1, 2)[:self.V]
        s = np.zeros(self.V, dtype=np.uint32)
        s[:len(r)] = r[:, 0]
        s[:len(r)][(r[:, 0] == 0) & (r[:, 1] == vo.MAX_INT32)] = FORK_SEQ
        return s

    def process(self, evs, flags):
        for ev, f in zip(evs, flags):
            s = self.seqs(ev)
            self.mt[int(self.creator[ev])] = s
            if f:
                self.sp = s

    def matrix(self):
        return self.mt.T                                        # [validator, creator]

    def medians(self, rows=None):
        """Per row: stable argsort by seq descending (as one sort of
        (~seq, index) keys), cumsum of weights, first position >= quorum."""
        m = self.matrix() if rows is None else self.matrix()[np.asarray(rows)]
        out = np.zeros(len(m), dtype=np.uint32)
        col = np.arange(self.V, dtype=np.uint64)
        for lo in range(0, len(m), 512):                         # (bounds the temporaries)
            c = m[lo:lo + 512]
            key = np.sort((np.uint64(0xFFFFFFFF) - c.astype(np.uint64)) << np.uint64(32) | col, axis=1)
            order = (key & np.uint64(0xFFFFFFFF)).astype(np.int64)
            k = np.argmax(np.cumsum(self.w[order], axis=1) >= self.quorum, axis=1)
            out[lo:lo + 512] = np.take_along_axis(c, order, axis=1)[np.arange(len(c)), k]
        return out

    def metric(self, ev, cap, med=None):
        """GetMetricOf with the capped difference; the sum in Python ints mod 2^64."""
        med = (self.medians() if med is None else med).astype(np.int64)
        upd, cur, w = self.seqs(ev).astype(np.int64), self.sp.astype(np.int64), self.w
        total = 0
        for i in np.flatnonzero((upd > med) & (upd > cur)).tolist():
            m, c, u, wi = int(med[i]), int(cur[i]), int(upd[i]), int(w[i])
            x = min(u - m, cap) * wi
            if m < c:
                x -= min(c - m, cap) * wi
            total += x
        return total & MASK64


def oracle_of(w, arrays):
    o = corc.OracleIndex(w)
    assert o.add_batch(*arrays) == -1
    return o


def qi_hub(V):
    """The chain's creator in the QuorumIndexer cases: not lane 0 of the
    metric's wave where the width allows."""
    return min(V - 1, 37)


def quorum_edge_cases(d, w):
    """(name, events to process, row u, what its median must be): creator
    subsets of weight Q - 1, Q, Q + 1 whose events all observe root u, taken
    from the start, the end and the middle of the index range."""
    Q = quorum_of(w)
    u = d.others[0] if d.others else d.hub
    ev_of = dict(d.layer2)
    ev_of[d.hub] = d.chain[0]
    out = []
    for where in ("start", "end", "middle"):
        order = placed_order(list(range(d.V)), where)
        for step in (-1, 0, 1):
            if Q + step > sum(w):
                continue                                         # (V = 1: Q is the whole weight)
            S = subset_with_sum(w, Q + step, order)
            out.append(("%s%+d" % (where, step), [ev_of[c] for c in S], u, S, Q + step))
    return out


def whole_matrix_plan(d, me):
    """Events in processing order with their self flags: every second-layer
    event, chain events interleaved (the hub's later event wins, and the last
    is not the newest), some roots after their creator's second-layer event
    (the older event wins), self flags on validator `me`'s events."""
    evs = []
    chain = list(d.chain[::-1]) + ([d.chain[len(d.chain) // 2]] if len(d.chain) > 1 else [])
    step = max(1, len(d.others) // max(1, len(chain)))
    for k, v in enumerate(d.others):
        evs.append(d.layer2[v])
        if k % step == 0 and chain:
            evs.append(chain.pop(0))
        if k % 5 == 3:
            evs.append(v)                                        # its root, again
    evs.extend(chain)
    if not evs:
        evs = [d.chain[0]]
    return evs, [1 if d.creator[e] == me else 0 for e in evs]


def batches(evs, flags):
    """Batches of 1, 16, 17 and all that is left."""
    i, out = 0, []
    for n in BATCHES:
        if i < len(evs):
            out.append((evs[i:i + n], flags[i:i + n]))
            i += n
    if i < len(evs):
        out.append((evs[i:], flags[i:]))
    return out


def metric_plan(d):
    """Processed: every second-layer event, then c_1 as the self event.
    Candidates: the chain.  With heavy_weights(V, hub) row hub's median is the
    hub's own seq 2, and c_j gains (j - 1) * w_hub."""
    evs = [d.layer2[v] for v in d.others] + [d.chain[0]]
    return evs, [0] * len(d.others) + [1], list(d.chain)
