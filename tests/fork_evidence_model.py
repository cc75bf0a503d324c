"""CPU model of fork evidence (include/lachesis_ancestry.h, lx_anc_fork_pairs /
lx_anc_cheaters) over :class:`ancestry_model.Model`.

*naive*  : the reference's own definition of a fork, the "naive implementation
  of fork detection" of testForksDetected (vecfc/forkless_cause_test.go:
  490-518): head observes a fork of creator c <=> two different events of c
  with the same seq are head or ancestors of head.  With S(head, c) = those
  events, the canonical answer is ``(x, y, seq*)``: seq* the lowest seq two
  events of S share, x < y the two lowest dense indices of S at seq*;
  ``(NONE, NONE, 0)`` where there is none.  :func:`evidence_row` buckets the
  ancestor bitset of one head by (creator, seq).

*rule*   : what the kernel computes, on the C oracle's rows: head's view of a
  branch is an interval of seqs whose end is the number of the branch's events
  that pass ``x <= head and 0 < LA(x)[branch(head)] <= seq(head)`` (monotone
  along the branch); seq* is the lowest first seq of an interval that another
  interval of the same creator covers.

Dense indices and creator idxs throughout.
"""

import numpy as np

NONE = 0xFFFFFFFF
NO_EVIDENCE = (NONE, NONE, 0)


def evidence_row(m, head):
    """{creator idx: (x, y, seq*)} for every creator head has evidence of."""
    slots = {}
    bits = bin(m.anc[head])[:1:-1]
    for e, bit in enumerate(bits):
        if bit == "1":
            slots.setdefault((int(m.creator[e]), int(m.seq[e])), []).append(e)
    out = {}
    for (c, s), evs in slots.items():
        if len(evs) >= 2 and (c not in out or s < out[c][2]):
            out[c] = (evs[0], evs[1], s)                     # (ascending: e counts up)
    return out


def evidence(m, head, creator):
    return evidence_row(m, head).get(int(creator), NO_EVIDENCE)


def evidence_all(m, heads=None):
    """(x, y, seq) arrays [len(heads), V] for every head x creator."""
    heads = range(m.n) if heads is None else heads
    V = len(m.validators.weights)
    x = np.full((len(heads), V), NONE, dtype=np.uint32)
    y = np.full((len(heads), V), NONE, dtype=np.uint32)
    s = np.zeros((len(heads), V), dtype=np.uint32)
    for k, h in enumerate(heads):
        for c, (a, b, q) in evidence_row(m, int(h)).items():
            x[k, c], y[k, c], s[k, c] = a, b, q
    return x, y, s


def cheaters(m, head):
    """lx_anc_cheaters of one head: [(creator, x, y, seq)], ascending creator."""
    return [(c,) + t for c, t in sorted(evidence_row(m, int(head)).items())]


def max_slot(m):
    """The most events of one creator with one seq."""
    n = {}
    for c, s in zip(m.creator, m.seq):
        n[(int(c), int(s))] = n.get((int(c), int(s)), 0) + 1
    return max(n.values())


# ---- the branch-interval rule on the oracle's rows

class Branches:
    """The branch tables of the index, from the oracle's branch of every event:
    ``events[b]`` in seq order (consecutive seqs), ``first[b]``, and per creator
    idx its branches, the original first."""

    def __init__(self, m):
        _, branch, _, _, _ = m.rows()
        B = int(branch.max()) + 1
        self.events = [[] for _ in range(B)]
        for e in range(m.n):
            self.events[int(branch[e])].append(e)
        self.first = []
        self.of_creator = {}
        for b, evs in enumerate(self.events):
            if not evs:                                      # (a validator without events)
                self.first.append(1)
                continue
            sq = [int(m.seq[e]) for e in evs]
            assert sq == list(range(sq[0], sq[0] + len(evs)))    # a chain of consecutive seqs, in Add order
            assert len({int(m.creator[e]) for e in evs}) == 1
            self.first.append(sq[0])
            self.of_creator.setdefault(int(m.creator[evs[0]]), []).append(b)


def observed_counts(m, br):
    """[head, branch]: how many events of the branch pass the LowestAfter rule
    for head; asserts that they are a prefix of the branch (monotone)."""
    obs = np.tril(m.la_rule_matrix())                        # x <= head
    cnt = np.zeros((m.n, len(br.events)), dtype=np.int64)
    for b, evs in enumerate(br.events):
        if not evs:
            continue
        sub = obs[:, evs]
        assert (sub[:, 1:] <= sub[:, :-1]).all(), b
        cnt[:, b] = sub.sum(axis=1)
    return cnt


def interval_rule(br, cnt_row, creator):
    """The kernel's answer for one head (its row of :func:`observed_counts`)."""
    iv = [(br.first[b], br.first[b] + int(cnt_row[b]) - 1, b) for b in br.of_creator.get(creator, [])
          if cnt_row[b] > 0]
    best = None
    for j, (fj, _, _) in enumerate(iv):
        if any(i != j and fi <= fj <= hi for i, (fi, hi, _) in enumerate(iv)):
            best = fj if best is None else min(best, fj)
    if best is None:
        return NO_EVIDENCE
    evs = sorted(br.events[b][best - f] for f, hi, b in iv if f <= best <= hi)
    return (evs[0], evs[1], best)


def sweep_rule(br, cnt_row, creator):
    """The same by the sweep of the intervals sorted by first seq: seq* is the
    first first_j that the highest end seen so far reaches."""
    iv = sorted((br.first[b], br.first[b] + int(cnt_row[b]) - 1) for b in br.of_creator.get(creator, [])
                if cnt_row[b] > 0)
    top = -1
    for f, hi in iv:
        if top >= f:
            return f
        top = max(top, hi)
    return None
