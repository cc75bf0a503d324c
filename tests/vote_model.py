"""Plain reference of the election's vote kernels: election_math.go:13-114
applied to an observe relation, for all root slots of a frame at once, in the
vote / decision / error words of lx_abft_kernels.hip (k_vote_init,
k_vote_round1, k_vote_round).  numpy with 64-bit integers; no GPU.

A relation (``Relation``) is what tests/csrc/vote_harness.cpp takes: frames
k = 0..G with their root slots (event id or NONE, creator idx, ``dup`` = the
previous slot of the same creator in the frame or NONE) and, for every slot of
a frame k >= 1, the set of slots of frame k - 1 it observes (forkless-causes).
Election e decides frame e and votes in frames e + 1 .. G (round k - e).

The reference asks a root only about the subjects not decided yet and stops
once the Atropos is known; the kernels answer every subject of the window for
every slot (their contract), and so does this model: the reference's three
checks -- an observed root without a vote, two observed roots of one validator
or two yes-votes naming different roots, observed stake below the quorum --
are evaluated for every (slot, subject) and OR-ed into the election's error
word.  Sums are not de-duplicated by validator: two observed roots of one
validator are an error already.  Where kVoteErrTwoRoots is raised by differing
yes-votes, the observed root a slot reports for that subject is the kernel's
business (the reference has panicked): compare the error word only.
"""

import numpy as np

NONE = 0xFFFFFFFF
VOTED, YES, DECIDED, NOROOT = 0x80000000, 0x40000000, 0x20000000, 0x1FFFFFFF
ERR_MISSING, ERR_TWO_ROOTS, ERR_QUORUM = 1, 2, 4
UNDECIDED = 0xFFFFFFFFFFFFFFFF


class Relation:
    def __init__(self, weights, quorum=None):
        self.w = np.asarray(weights, dtype=np.int64)
        self.V = len(self.w)
        total = int(self.w.sum())
        self.quorum = total * 2 // 3 + 1 if quorum is None else quorum
        self.ev, self.creator, self.dup, self.obs = [], [], [], []

    def add_frame(self, ev, creator, obs=None):
        """Slots in list order; obs = bool [slots][slots of the frame before]
        (None for frame 0).  ``dup`` follows from the creators."""
        ev = np.asarray(ev, dtype=np.int64)
        creator = np.asarray(creator, dtype=np.int64)
        dup = np.full(len(ev), NONE, dtype=np.int64)
        last = {}
        for i, c in enumerate(creator.tolist()):
            dup[i] = last.get(c, NONE)
            last[c] = i
        k = len(self.ev)
        n_prev = len(self.ev[-1]) if k else 0
        obs = np.zeros((len(ev), n_prev), dtype=bool) if obs is None else np.asarray(obs, dtype=bool)
        assert obs.shape == (len(ev), n_prev)
        self.ev.append(ev)
        self.creator.append(creator)
        self.dup.append(dup)
        self.obs.append(obs)
        return self

    @property
    def G(self):
        return len(self.ev) - 1


def tables(rel, E, stride):
    """[(e, k)] in the harness's order and the offset of each in the flat votes array."""
    out, off, tot = [], {}, 0
    for e in range(E):
        for k in range(e + 1, rel.G + 1):
            out.append((e, k))
            off[(e, k)] = tot
            tot += len(rel.ev[k]) * stride
    return out, off, tot


def _launch(rel, e, k, votes, dec, v_lo, v_hi, lo, hi):
    """One launch_votes: slots [lo, hi) of frame k, subjects [v_lo, v_hi).
    Returns the error bits."""
    t = votes[(e, k)]
    t[lo:hi, v_lo:v_hi] = VOTED | NOROOT                       # k_vote_init
    live = np.nonzero(rel.ev[k][lo:hi] != NONE)[0] + lo
    obs, pc = rel.obs[k], rel.creator[k - 1]
    err = 0
    if k == e + 1:                                             # k_vote_round1
        for r in range(obs.shape[1]):                          # list order: the last root of a validator wins
            c = pc[r]
            if v_lo <= c < v_hi:
                t[live[obs[live, r]], c] = VOTED | YES | r
        return 0
    prev = votes[(e, k - 1)][:, v_lo:v_hi]                     # [slots of k - 1][subjects]
    wc = rel.w[pc]
    pdup = rel.dup[k - 1]
    py = (prev & YES) != 0
    ix = prev & NOROOT
    unvoted = ((prev & VOTED) == 0).any(axis=1)
    big = np.int64(1) << 40
    ix_lo, ix_hi = np.where(py, ix, big), np.where(py, ix, -1)
    # subjects whose yes-votes of the whole frame name one root (all of them,
    # but for fork roots): every slot sees that root or none
    col_lo, col_hi = ix_lo.min(axis=0, initial=big), ix_hi.max(axis=0, initial=-1)
    mixed = np.nonzero((col_hi >= 0) & (col_lo != col_hi))[0]
    pyw = py * wc[:, None]
    for s in live:
        rs = np.nonzero(obs[s])[0]
        for r in (rs if (pdup != NONE).any() else ()):         # allVotes.Count == false
            d = pdup[r]
            while d != NONE:
                if obs[s, d]:
                    err |= ERR_TWO_ROOTS
                d = pdup[d]
        if unvoted[rs].any():
            err |= ERR_MISSING
        yes = pyw[rs].sum(axis=0)
        no = int(wc[rs].sum()) - yes
        any_yes = py[rs].any(axis=0)
        subj = np.where(any_yes, col_hi, NOROOT)
        if len(mixed):
            lo = ix_lo[np.ix_(rs, mixed)].min(axis=0, initial=big)
            hi = ix_hi[np.ix_(rs, mixed)].max(axis=0, initial=-1)
            if ((hi >= 0) & (lo != hi)).any():
                err |= ERR_TWO_ROOTS
            subj[mixed] = np.where(hi >= 0, hi, NOROOT)
        if int(wc[rs].sum()) < rel.quorum:
            err |= ERR_QUORUM
        y = yes >= no
        decided = (yes >= rel.quorum) | (no >= rel.quorum)
        o = np.where(y, subj, NOROOT)
        t[s, v_lo:v_hi] = VOTED | np.where(y, YES, 0) | np.where(decided, DECIDED, 0) | o
        word = (np.uint64(int(rel.ev[k][s])) << np.uint64(32)) | np.where(y, 1 << 31, 0).astype(np.uint64) | o.astype(np.uint64)
        cur = dec[e][v_lo:v_hi]
        dec[e][v_lo:v_hi] = np.where(decided, np.minimum(cur, word), cur)
    return err


def run(rel, E=1, stride=None, steps=None, merged=False):
    """What vh_run returns: (votes {(e, k): int64 [slots][stride]}, dec uint64
    [E][stride], err [E]).  steps = [(v_lo, v_hi, slot_from, slot_to)]."""
    stride = rel.V if stride is None else stride
    steps = [(0, stride, 0, 1 << 30)] if steps is None or merged else steps
    order, _, _ = tables(rel, E, stride)
    votes = {ek: np.zeros((len(rel.ev[ek[1]]), stride), dtype=np.int64) for ek in order}
    dec = np.full((E, stride), UNDECIDED, dtype=np.uint64)
    err = np.zeros(E, dtype=np.uint32)
    for e in range(E):
        for v_lo, v_hi, lo, hi in steps:
            for k in range(e + 1, rel.G + 1):
                n = len(rel.ev[k])
                lo_, hi_ = min(lo, n), min(hi, n)
                if lo_ < hi_:
                    err[e] |= _launch(rel, e, k, votes, dec, v_lo, v_hi, lo_, hi_)
    return votes, dec, err


def atropos_state(dec_row, vw=None):
    """chooseAtropos (sort_roots.go:10-25) over decision words in idx order:
    ("pending",), ("all_no",) or ("decided", event that decided, slot of the Atropos)."""
    tmax = 0
    for word in dec_row[:vw].tolist():
        if word == UNDECIDED:
            return ("pending",)
        tmax = max(tmax, word >> 32)
        if word & 0x80000000:
            return ("decided", tmax, word & NOROOT)
    return ("all_no",)


# ---------------------------------------------------------------------------- relations

def golden_case(c, order_seed):
    """A TestProcessRoot case (tests/golden/abft_golden.json election_cases,
    election_test.go:172-285) as (validators, events in processing order,
    frame per event id, observe edges).  order_seed 0: scheme order; else a
    random topological order (reorder() of the reference's test)."""
    from abft_harness import topo_shuffle
    from oracle import abft_oracle as ao
    from oracle import pos, tdag
    frame_of, edges, ordered = {}, set(), []

    def process(e, name):
        frame_of[e.id] = int(name.split("_")[1])
        sp = ao.self_parent(e)
        for p in e.parents:
            if not (p == sp and name.startswith("+")):
                edges.add((e.id, p))
        ordered.append(e)

    nodes, _, _, _ = tdag.ascii_scheme_for_each(c["scheme"], process)
    first = {}
    for e in ordered:
        first.setdefault(e.creator, e.name.lstrip("+"))
    validators = pos.Validators({v: c["weights"]["node" + first[v][0].upper()] for v in nodes})
    order = topo_shuffle(ordered, tdag.SplitMix64(order_seed)) if order_seed else ordered
    return validators, order, frame_of, edges


def relation_of(validators, order, frame_of, edges):
    """The Relation of events processed in ``order``: event id = position in
    the order, a frame's slots in that order."""
    rel = Relation(validators.weights, validators.quorum())
    prev = []
    for k in range(max(frame_of.values()) + 1):
        cur = [(i, e) for i, e in enumerate(order) if frame_of[e.id] == k]
        obs = [[(e.id, p.id) in edges for _, p in prev] for _, e in cur]
        rel.add_frame([i for i, _ in cur], [validators.idxs[e.creator] for _, e in cur], obs if k else None)
        prev = cur
    return rel


def reference_election(validators, order, frame_of, edges):
    """oracle.abft_oracle.Election fed the roots in ``order``: (election,
    result or None, position of the root at which it first answered)."""
    from oracle import abft_oracle as ao
    roots = {e.id: ao.RootAndSlot(e.id, frame_of[e.id], e.creator) for e in order}
    by_frame = {}
    for e in order:
        by_frame.setdefault(frame_of[e.id], []).append(roots[e.id])
    el = ao.Election(validators, 0, lambda a, b: (a, b) in edges, lambda f: by_frame.get(f, []))
    res, at = None, None
    for i, e in enumerate(order):
        got = el.process_root(roots[e.id])
        if got is not None and res is None:
            res, at = got, i
    return el, res, at


def random_case(V, seed, frames=6, p_root=0.85, p_extra=0.3):
    """An error-free random relation as golden_case returns one: random
    weights, some validators without a root in a frame, one root per validator
    and frame at most, every root observing at least quorum stake of the
    frame before."""
    from oracle import pos, tdag
    rng = np.random.default_rng(seed)
    validators = pos.Validators({v + 1: int(x) for v, x in enumerate(rng.integers(1, 1000, V))})
    w = dict(zip(validators.ids, validators.weights))
    order, frame_of, edges, prev = [], {}, set(), []
    for k in range(frames):
        while True:
            cur = [v for v in validators.ids if rng.random() < p_root]
            if sum(w[v] for v in cur) >= validators.quorum():
                break
        cur = [cur[i] for i in rng.permutation(len(cur))]
        now = []
        for v in cur:
            e = tdag.Event(len(order) + 1, v, k + 1, k + 1, [])
            frame_of[e.id] = k
            got = 0
            for j, i in enumerate(rng.permutation(len(prev)) if prev else []):
                if got < validators.quorum() or rng.random() < p_extra:
                    edges.add((e.id, prev[i].id))
                    got += w[prev[i].creator]
            order.append(e)
            now.append(e)
        prev = now
    return validators, order, frame_of, edges
