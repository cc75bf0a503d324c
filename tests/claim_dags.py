"""Claimed-frame batches with low, wrong, inflated and post-seal claims
(tests/test_claim_dags.py, tests/test_gpu_abft_claims.py).

Process takes an event's claimed frame as the bound of calcFrameIdx's loop
(abft/event_processing.go:163-189), so a root claiming less than its true
frame -- down to its self-parent's frame, which denies that it is a root -- is
accepted, and the epoch goes on with other roots, frames and blocks.  A claim
that is wrong in any other way is refused, at the event or (when an accepted
under-claim moved a later event's true frame) at an honest event behind it.

Every generator here is seeded (SplitMix64), works on the events of
``tdag.rand_fork_dag`` and returns claim vectors together with the verdict of
the oracle, ``abft_harness.FakeLachesis`` driven event by event
(``mass_return``, honest claims over the step budget of one pass, is an
``election_dags.scheduled`` DAG for the C oracle).  Plain Python: importable
without a GPU.
"""

from oracle import abft_oracle as ao
from oracle import tdag
from oracle.tdag import SplitMix64
from abft_harness import FakeLachesis, node_ids

FRAME_BUILD = 0xFFFFFFFF

SHAPES = {
    # weights, cheaters, events/node, parents, seed
    "A": ([1, 1, 1, 1], 0, 30, 3, 21),
    "B": ([1, 2] * 5, 3, 30, 5, 6),
    "C": ([11, 11, 11, 67], 0, 40, 4, 3),      # one validator alone holds the quorum
    "D": ([5 + (i % 7) for i in range(40)], 4, 15, 8, 8),
}
LOW_MODES = [(3, 1), (2, "spf"), (5, 1)]
KINDS = ["-2", "-1", "+1", "+2", "spf", "0", "top+1", "top+2", "max"]
N_CASES = 36


def gen_events(weights, cheaters, events_per_node, parent_count, seed, forks=10, eid_base=0):
    nodes = node_ids(len(weights), seed=seed)
    _, evs = tdag.rand_fork_dag(len(nodes), events_per_node, parent_count, cheaters=cheaters, forks_count=forks,
                                node_ids=nodes, rng=SplitMix64(seed), eid_base=eid_base)
    return nodes, evs


def shape_events(shape):
    """(weights by node id, fresh events) of a named shape."""
    weights, cheaters, epn, pc, seed = SHAPES[shape]
    nodes, evs = gen_events(weights, cheaters, epn, pc, seed)
    return dict(zip(nodes, weights)), evs


def snapshot(o):
    return dict(blocks=list(o.block_list), last=(o.store.get_epoch(), o.store.last_decided_frame))


_honest = {}


def honest(shape):
    """Build + Process per event: frames {event id: frame}, blocks, last."""
    if shape not in _honest:
        wmap, evs = shape_events(shape)
        o = FakeLachesis(wmap)
        for e in evs:
            o.build(e)
            assert o.process(e) is None
        _honest[shape] = dict(frames={e.id: e.frame for e in evs}, **snapshot(o))
    return _honest[shape]


def lowballed(shape, every, drop):
    """The epoch in which every ``every``-th root (of those with a self-parent)
    claims its frame less one (drop 1) or its self-parent's frame ("spf"):
    Build, lower, Process, event by event.  ``claims`` are the frames the
    oracle accepted ({event id: frame}; ``err`` is None when it accepted all
    of them), ``lowered`` counts the lowered ones."""
    wmap, evs = shape_events(shape)
    o = FakeLachesis(wmap)
    claims, roots, lowered, err = {}, 0, 0, None
    for e in evs:
        o.build(e)
        sp = ao.self_parent(e)
        if sp is not None and e.frame != claims[sp]:
            roots += 1
            if roots % every == 0:
                e.frame = claims[sp] if drop == "spf" else e.frame - 1
                lowered += 1
        err = o.process(e)
        if err is not None:
            break
        claims[e.id] = e.frame
    return dict(claims=claims, frames=dict(claims), lowered=lowered, err=err, n=len(evs), **snapshot(o))


def _claim_of(kind, i, evs, hon):
    """The claim of kind ``kind`` for event i of an honest epoch."""
    h = hon[evs[i].id]
    sp = ao.self_parent(evs[i])
    top = max([hon[e.id] for e in evs[:i]], default=0)
    return {"-2": h - 2, "-1": h - 1, "+1": h + 1, "+2": h + 2, "spf": hon[sp] if sp is not None else 0, "0": 0,
            "top+1": top + 1, "top+2": top + 2, "max": 0xFFFFFFFE}[kind]


def drive_claimed(o, evs, claims):
    """Process per event on the given claims until the first error: the
    number of events consumed."""
    for i, e in enumerate(evs):
        e.frame = claims[e.id]
        if o.process(e) is not None:
            return i
    return len(evs)


def drive_build(o, evs):
    for e in evs:
        o.build(e)
        assert o.process(e) is None


_mutated = {}


def mutated(shape, case):
    """One to three events of the honest epoch claim a frame of one of KINDS
    (every sixth case the first of them is a creator's first event, one
    without a self-parent; draws that equal the honest frame or are negative
    are skipped).  The oracle's verdict: ``consumed`` (= the position of the
    rejected event, or n), the frames of the consumed events, the blocks so
    far; then ``final``: blocks and last decided frame once everything from
    the rejected event on was processed with Build semantics."""
    key = (shape, case)
    if key in _mutated:
        return _mutated[key]
    wmap, evs = shape_events(shape)
    hon = honest(shape)["frames"]
    rng = SplitMix64(1000 * (ord(shape) - ord("A")) + case + 77)
    n = len(evs)
    firsts = [i for i, e in enumerate(evs) if ao.self_parent(e) is None]
    claims = dict(hon)
    muts = {}
    want = 1 + rng.below(3)
    while len(muts) < want:
        if case % 6 == 5 and not muts:
            i = firsts[rng.below(len(firsts))]
        else:
            i = rng.below(n)
        kind = KINDS[rng.below(len(KINDS))]
        c = _claim_of(kind, i, evs, hon)
        if i in muts or c < 0 or c == hon[evs[i].id]:
            continue
        muts[i] = kind
        claims[evs[i].id] = c
    o = FakeLachesis(wmap)
    consumed = drive_claimed(o, evs, claims)
    res = dict(claims=claims, muts=muts, n=n, consumed=consumed, frames={e.id: e.frame for e in evs[:consumed]},
               **snapshot(o))
    if consumed == n:
        res["outcome"] = "accepted"
    elif consumed in muts:
        res["outcome"] = "at_mutated"
    elif consumed > max(muts):
        res["outcome"] = "later"
    else:
        res["outcome"] = "between"
    drive_build(o, evs[consumed:])
    res["final"] = snapshot(o)
    _mutated[key] = res
    return res


LADDER_SEED = 41
_ladder = {}


def ladder_events(V):
    wmap = {k + 1: 1 + k % 5 for k in range(V)}
    _, evs = tdag.rand_fork_dag(V, 4, 6, seed=LADDER_SEED)
    return wmap, evs


def ladder(V):
    """rand_fork_dag(V, 4, 6) with honest frames, and its last V events (one
    per validator, every self-parent before them) claiming top + 1 + k, top =
    the highest honest frame before them.  ``steps`` = the frame steps these
    claims ask for, sum(claim - selfParentFrame); ``consumed`` = where the
    oracle refuses the round (position within it) after the honest prefix."""
    if V in _ladder:
        return _ladder[V]
    wmap, evs = ladder_events(V)
    o = FakeLachesis(wmap)
    drive_build(o, evs)
    hon = {e.id: e.frame for e in evs}
    full = snapshot(o)
    prefix, rnd = evs[:-V], evs[-V:]
    assert sorted(e.creator for e in rnd) == sorted(wmap) and all(ao.self_parent(e) is not None for e in rnd)
    top = max(hon[e.id] for e in prefix)
    claims = dict(hon)
    for k, e in enumerate(rnd):
        claims[e.id] = top + 1 + k
    steps = sum(claims[e.id] - hon[ao.self_parent(e)] for e in rnd)
    o = FakeLachesis(wmap)
    assert drive_claimed(o, prefix, hon) == len(prefix)
    consumed = drive_claimed(o, rnd, claims)
    _ladder[V] = dict(V=V, n=len(evs), honest=hon, claims=claims, top=top, steps=steps, consumed=consumed,
                      frames={e.id: e.frame for e in rnd[:consumed]}, full=full, **snapshot(o))
    return _ladder[V]


TAIL_KINDS = ["honest", "one", "top2", "build"]
TAIL_SHAPE = ([1, 2] * 5, 0, 60, 5, 11)
TAIL_SEAL_FRAME = 3
TAIL_BAD = 90
_tail = {}


def tail_events():
    nodes, evs = gen_events(*TAIL_SHAPE)
    return dict(zip(nodes, TAIL_SHAPE[0])), evs


def tail_epoch2():
    """A small honest DAG of the epoch after the seal (same validators)."""
    nodes = node_ids(len(TAIL_SHAPE[0]), seed=TAIL_SHAPE[4])
    _, evs = tdag.rand_fork_dag(len(nodes), 10, 5, node_ids=nodes, rng=SplitMix64(12), eid_base=10**6)
    for e in evs:
        e.epoch = 2
    return evs


def seal_at(t, frame):
    """Makes the harness seal the epoch (validators unchanged) when ``frame``
    is decided."""
    def apply_block(block):
        if t.store.last_decided_frame + 1 == frame:
            return t.store.get_validators()
        return None
    t.apply_block = apply_block


def sealed_tail(kind):
    """One batch with a seal inside: the epoch is sealed when frame 3 is
    decided, at event ``seal_pos``; the events behind it claim what an
    unsealed honest run gives them ("honest"), 1 ("one"), the same with
    top + 2 on event 90 alone ("top2"), or LX_FRAME_BUILD ("build").  The
    oracle stops at the seal and never looks at them: blocks and epoch there,
    then the blocks of an honest epoch-2 DAG processed afterwards."""
    if kind in _tail:
        return _tail[kind]
    wmap, evs = tail_events()
    o = FakeLachesis(wmap)
    drive_build(o, evs)
    unsealed = {e.id: e.frame for e in evs}
    o = FakeLachesis(wmap)
    seal_at(o, TAIL_SEAL_FRAME)
    consumed, err = o.process_batch(evs, claimed=True)
    assert err is None
    claims = dict(unsealed)
    for i, e in enumerate(evs[consumed:], consumed):
        if kind == "one":
            claims[e.id] = 1
        elif kind == "build":
            claims[e.id] = FRAME_BUILD
        elif kind == "top2" and i == TAIL_BAD:
            claims[e.id] = max(unsealed[x.id] for x in evs[:i]) + 2
    res = dict(claims=claims, n=len(evs), consumed=consumed, seal_pos=consumed - 1, **snapshot(o))
    o.apply_block = None
    e2 = tail_epoch2()
    c2, err = o.process_batch(e2, claimed=False)
    assert err is None and c2 == len(e2)
    res["epoch2"] = dict(frames={e.id: e.frame for e in e2}, **snapshot(o))
    _tail[kind] = res
    return res


def pass_budget(n, V):
    """Frame steps one pass of a claimed batch may queue before it is cut
    (include/lachesis_abft.h, lx_abft_process_batch): n events of the call."""
    return 2 * n + 4 * V + 64


def claimed_steps(d, frames, lo, hi):
    """sum(claim - selfParentFrame) over the events [lo, hi) of a dense DAG."""
    steps = 0
    for i in range(lo, hi):
        if d.seq[i] > 1 and d.poff[i + 1] > d.poff[i]:
            steps += int(frames[i]) - int(frames[int(d.par[int(d.poff[i])])])
    return steps


RETURN_LEVEL = 80


def mass_return():
    """(weights, dag, lo, hi): ten heavy validators carry the epoch alone
    while thirty light ones are silent from level 2 on; all thirty return in
    level RETURN_LEVEL = the events [lo, hi), each climbing from frame 1 to
    the top in one event -- honest claims that ask for more frame steps than
    one pass of the batch takes."""
    import election_dags as ed
    w = [10] * 10 + [1] * 30
    active = lambda l, v: v < 10 or l < 2 or l >= RETURN_LEVEL
    see = lambda l, v: range(10)
    d = ed.scheduled(len(w), 4, RETURN_LEVEL + 3, 5, active, see)
    return w, d, int(d.level_ends[RETURN_LEVEL]), int(d.level_ends[RETURN_LEVEL + 1])
