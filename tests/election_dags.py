"""Scheduled-participation DAGs for the election tests
(tests/test_election_dags.py, tests/test_gpu_election_dags.py).

A level-synchronous generator without forks: at level l every validator v with
``active(l, v)`` emits one event on its own last event and on the last events
of P - 1 distinct other validators, drawn from ``see(l, v)`` (default: every
validator that has an event) against a snapshot of the tips taken at the start
of the level.  Silent validators make the election take the branches a fully
participating network never does: with the heaviest 64 (or more) validators of
the idx order silent, every subject of the first vote window is decided "no"
and the Atropos is found only after the window was widened.  Plain numpy /
Python: importable without a GPU.
"""

import numpy as np

from lachesis_hip.tools import Dag
from oracle.tdag import SplitMix64


def scheduled(V, P, levels, seed, active=None, see=None):
    """Dense arrays in Add order (level by level, validator idx order within a
    level).  The returned Dag also carries ``level`` (per event) and
    ``level_ends`` (events up to and including level l, ``level_ends[0]`` = 0
    and ``level_ends[l + 1]`` after level l)."""
    rng = SplitMix64(seed)
    creator, seq, lam, level, poff, par = [], [], [], [], [0], []
    last = [-1] * V
    ends = [0]
    for l in range(levels):
        tips = list(last)
        have = [v for v in range(V) if tips[v] >= 0]
        for v in range(V):
            if active is not None and not active(l, v):
                continue
            pool = [o for o in (have if see is None else see(l, v)) if o != v and tips[o] >= 0]
            k = min(P - 1, len(pool))
            for i in range(k):   # partial Fisher-Yates: k distinct draws
                j = i + rng.below(len(pool) - i)
                pool[i], pool[j] = pool[j], pool[i]
            ps = ([tips[v]] if tips[v] >= 0 else []) + [tips[o] for o in pool[:k]]
            last[v] = len(creator)
            creator.append(v)
            seq.append(seq[tips[v]] + 1 if tips[v] >= 0 else 1)
            lam.append(1 + max((lam[p] for p in ps), default=0))
            level.append(l)
            par.extend(ps)
            poff.append(len(par))
        ends.append(len(creator))
    d = Dag(np.array(creator, dtype=np.uint32), np.array(seq, dtype=np.uint32), np.array(lam, dtype=np.uint32),
            np.array(poff, dtype=np.uint64), np.array(par if par else [0], dtype=np.uint32), V)
    d.level = np.array(level, dtype=np.uint32)
    d.level_ends = np.array(ends, dtype=np.int64)
    return d


# OUTAGE = the levels [lo, hi) on which the head of head_silent_return is silent
OUTAGE = (8, 28)
# seeds with the longest elections of seeds 0..79 (V 4: one of 9 rounds, past
# the 8 rounds elect_ahead may take, and six of >= 4; V 5: 5 rounds; V 7: 4)
LONG_SEED = {4: 76, 5: 71, 7: 73}
# weights [3, 3, 2, 2], the longest of seeds 0..199: 7 rounds, six of >= 4
UNEQUAL_SEED = 166


def scenario(name):
    """(weights, dag) of a named scenario."""
    if name == "head_silent_return":
        w, P, levels, seed = [1] * 200, 12, 40, 1
        active = lambda l, v: v >= 66 or not OUTAGE[0] <= l < OUTAGE[1]
    elif name == "head_never":
        w, P, levels, seed = [1] * 200, 12, 24, 2
        active = lambda l, v: v >= 66
    elif name == "head_never_two":
        w, P, levels, seed = [1] * 400, 16, 20, 3
        active = lambda l, v: v >= 130
    elif name == "lagger_return":
        # validator 3 silent on levels 9..11: its first event after them is the
        # first root to decide election 3 within two rounds, but younger than
        # a root of frame 6 that decides it in round 3 (test_election_dags.py)
        w, P, levels, seed = [1] * 4, 3, 40, 4
        active = lambda l, v: v != 3 or not 9 <= l < 12
    elif name == "long_rounds_weighted":
        # the golden "4rounds" weights: validator 0 is in every quorum (6 of
        # 8), so every root of frame F + 1 votes yes on subject 0 and every
        # election of a real DAG ends in round 2 -- long elections under unequal
        # weights need a set without such a validator (long_rounds_unequal)
        w, P, levels, seed, active = [4, 2, 1, 1], 3, 60, 0, None
    elif name == "long_rounds_unequal":
        w, P, levels, seed, active = [3, 3, 2, 2], 3, 60, UNEQUAL_SEED, None
    elif name.startswith("long_rounds"):
        V = int(name[len("long_rounds"):] or 4)
        w, P, levels, seed, active = [1] * V, 3, 60, LONG_SEED[V], None
    else:
        raise KeyError(name)
    return w, scheduled(len(w), P, levels, seed, active)


SCENARIOS = ["head_silent_return", "head_never", "head_never_two", "long_rounds", "long_rounds5", "long_rounds7",
             "long_rounds_weighted", "long_rounds_unequal", "lagger_return"]


def oracle_run(weights, dag, by_event=False, seal=None):
    """The C oracle's answer: frames, roots per frame, blocks, last decided
    frame; by_event also the election round counts {F: frame of the event at
    which block F was emitted - F} (one process_batch call per event).
    seal(epoch, frame) as corc.AbftOracle takes it: the run stops at the
    sealing event, ``consumed`` = the events of the sealed epoch."""
    from oracle import corc
    o = corc.AbftOracle(weights, seal=seal)
    n = len(dag)
    frames = np.zeros(n, dtype=np.uint32)
    rounds = {}
    for lo, hi in ([(i, i + 1) for i in range(n)] if by_event else [(0, n)]):
        nb = len(o.blocks)
        rc, consumed, out = o.process_batch(*dag.slice(lo, hi))
        assert rc == 0
        if consumed < hi - lo or o.epoch() != 1:
            frames[lo:lo + consumed] = out[:consumed]
            return dict(frames=frames[:lo + consumed], blocks=list(o.blocks), consumed=lo + consumed, epoch=o.epoch())
        frames[lo:hi] = out
        for b in o.blocks[nb:]:
            rounds[b[1]] = int(out[-1]) - b[1]
    nf = int(frames.max()) + 1
    return dict(frames=frames, roots=[o.frame_roots(f).tolist() for f in range(nf + 1)], blocks=list(o.blocks),
                last=o.last_decided_frame(), rounds=rounds)


def as_events(weights, dag):
    """The DAG as oracle.tdag events for abft_harness.FakeLachesis: validator
    ID = idx + 1 (idx order is weight desc, ID asc, so the scenario's weights
    must not increase), event ID = Add-order index + 1."""
    from oracle import tdag
    assert all(a >= b for a, b in zip(weights, weights[1:]))
    evs = []
    for i in range(len(dag)):
        ps = [int(p) + 1 for p in dag.par[int(dag.poff[i]):int(dag.poff[i + 1])]]
        e = tdag.Event(i + 1, int(dag.creator[i]) + 1, int(dag.seq[i]), int(dag.lamport[i]), ps)
        e.epoch = 1
        evs.append(e)
    return {v + 1: w for v, w in enumerate(weights)}, evs
