"""Two-speed DAGs whose fast validators reach seq 0x10000 cheaply, for the tests
of the 16-bit seq boundary (tests/test_gpu_seq16_boundary.py).

``F`` fast validators emit one event per level, the ``V - F`` slow ones one
event every ``every`` levels, so an epoch in which one creator has 65,536
events holds ~154k events at V = 24 instead of 1.5M.  Plain numpy / Python:
importable and buildable without a GPU or the tools library's generator.
"""

import numpy as np

from lachesis_hip.tools import Dag

L_LAST16 = 0xFFFF      # the last epoch length whose seqs all fit 16 bits
L_FIRST32 = 0x10000    # the first that does not
L_CROSS = 0x10028      # crosses the boundary, 40 levels past it
L_FAR = 0x10400        # several abft frames (~160 levels each) past it
CUT_BEFORE = 0xFFC0    # a batch cut 63 levels before the boundary

SMALL_W = {24: [3, 3] + [1] * 22, 12: [3, 3] + [1] * 10}
# every weight >= 2^16: the packed root-FC kernel's high-half dot products
WIDE_W = {24: [3 << 16] * 2 + [(1 << 16) | 5] * 22, 12: [3 << 16] * 2 + [(1 << 16) | 5] * 10}


def _distinct(rng, rows, n, m):
    """rows x m distinct draws from range(n) per row."""
    return np.argsort(rng.random((rows, n)), axis=1)[:, :m]


def two_speed(V, F, levels, every, seed, fork=False, base=None, base_level=0):
    """Level k = 1..levels: fast validator c (idx 0..F-1) emits one event on
    its self-parent and the latest event of fast validator (c + 1) % F, and
    when k % every == 1 also on the latest events of three random slow
    validators.  When k % every == 0 every slow validator (F..V-1) emits one
    event on its self-parent, the latest event of a random fast validator and
    the latest events of two random other slow ones.  seq = self-parent's + 1,
    Lamport = 1 + max over the parents; parents are distinct creators,
    self-parent first; a validator without an event yet is left out.

    fork: slow validator V-1 double-signs at level 2 * every -- a second event
    on the same self-parent with the same seq, whose only other parent is the
    latest event of fast validator 0.  Until V-1's next event the others see
    the second event as its latest while its own chain continues from the
    first, and fast validator 0 takes it as a parent at the next level, so
    both branches get observed and V-1 becomes a visible cheater.

    base / base_level: keep ``base``'s events up to level ``base_level`` and
    generate the levels after it from ``seed`` (a different continuation of
    the same prefix).

    The returned Dag also carries ``level`` (per event), ``level_ends``
    (events up to and including level k, for k = 0..levels), ``F`` and
    ``every``."""
    S = V - F
    assert F >= 2 and S >= 4 and levels >= 1
    rng = np.random.default_rng(seed)
    k0 = 0
    creator, seq, lam, level, poff, par = [], [], [], [], [0], []
    last = [-1] * V        # the event the others take as v's latest
    selfp = [-1] * V       # v's own chain tip (differs from last only after the double-sign)
    ends = [0]
    if base is not None:
        assert base.n_nodes == V and base.F == F and base.every == every
        assert 3 * every <= base_level <= len(base.level_ends) - 1
        k0 = base_level
        n0 = int(base.level_ends[k0])
        creator = base.creator[:n0].tolist()
        seq = base.seq[:n0].tolist()
        lam = base.lamport[:n0].tolist()
        level = base.level[:n0].tolist()
        poff = base.poff[:n0 + 1].tolist()
        par = base.par[:poff[-1]].tolist()
        ends = base.level_ends[:k0 + 1].tolist()
        for i, c in enumerate(creator):
            last[c] = selfp[c] = i
    n_wide = sum(1 for k in range(k0 + 1, levels + 1) if k % every == 1)
    n_slow = sum(1 for k in range(k0 + 1, levels + 1) if k % every == 0)
    fast_slow = F + _distinct(rng, max(n_wide, 1) * F, S, 3).reshape(-1, F, 3)
    slow_fast = rng.integers(0, F, (max(n_slow, 1), S))
    slow_slow = _distinct(rng, max(n_slow, 1) * S, S - 1, 2).reshape(-1, S, 2)
    i_wide = i_slow = 0

    def emit(c, others, k, sp=None):
        sp = selfp[c] if sp is None else sp
        ps = ([sp] if sp >= 0 else []) + [last[o] for o in others if last[o] >= 0]
        e = len(creator)
        creator.append(c)
        seq.append(seq[sp] + 1 if sp >= 0 else 1)
        lam.append(1 + max((lam[p] for p in ps), default=0))
        level.append(k)
        par.extend(ps)
        poff.append(len(par))
        return e

    for k in range(k0 + 1, levels + 1):
        wide = k % every == 1
        for c in range(F):
            others = [(c + 1) % F]
            if wide:
                others += [int(x) for x in fast_slow[i_wide, c]]
                if fork and c == 0 and k == 2 * every + 1 and V - 1 not in others:
                    others[-1] = V - 1     # the second branch is observed for certain
            last[c] = selfp[c] = emit(c, others, k)
        i_wide += wide
        if k % every == 0:
            for j in range(S):
                v = F + j
                oth = [F + int(x) + (int(x) >= j) for x in slow_slow[i_slow, j]]
                sp = selfp[v]
                last[v] = selfp[v] = emit(v, [int(slow_fast[i_slow, j])] + oth, k)
                if fork and v == V - 1 and k == 2 * every:
                    last[v] = emit(v, [0], k, sp=sp)
            i_slow += 1
        ends.append(len(creator))
    d = Dag(np.array(creator, dtype=np.uint32), np.array(seq, dtype=np.uint32), np.array(lam, dtype=np.uint32),
            np.array(poff, dtype=np.uint64), np.array(par, dtype=np.uint32), V)
    d.level = np.array(level, dtype=np.uint32)
    d.level_ends = np.array(ends, dtype=np.int64)
    d.F, d.every = F, every
    return d


def level_end(dag, k):
    """Number of events up to and including level k (= the fast validators' seq k)."""
    return int(dag.level_ends[k])


def queries(n, nq, span, seed):
    """ForklessCause pairs (a, b): b uniform over all n events for the first
    half of the queries and over the last 3000 events for the other half
    (the tail half); a = min(n - 1, b + U[0, span))."""
    rng = np.random.default_rng(seed)
    h = nq // 2
    b = np.concatenate([rng.integers(0, n, h), rng.integers(max(0, n - 3000), n, nq - h)])
    a = np.minimum(n - 1, b + rng.integers(0, span, nq))
    return a.astype(np.uint32), b.astype(np.uint32)


def fc_mix_ok(ans):
    """The oracle-side condition on a query set's answers: a true fraction
    within [0.2, 0.8] over all queries and over the tail half."""
    ans = np.asarray(ans)
    return all(0.2 <= float(x.mean()) <= 0.8 for x in (ans, ans[len(ans) // 2:]))
