"""Hand-built DAGs for fork evidence (tests/test_fork_evidence_model.py,
tests/test_gpu_fork_evidence.py), each with the answers it was built for.

Creator idx 0 is the cheater, the others observe: an observer's event has its
self-parent and at most one event of the cheater among its parents, so what a
head sees of each of the cheater's branches is exactly what the construction
says.  Event IDs are the dense indices (the events come in Add order), validator
id = idx + 1 with equal weights.

``DAGS[name]() -> Dag`` with ``cases = [(head, creator, (x, y, seq))]``,
``(NONE, NONE, 0)`` where the head has no evidence.  Plain Python, importable
without a GPU.
"""

from oracle import pos
from oracle.tdag import Event

from fork_evidence_model import NO_EVIDENCE


class Dag:
    def __init__(self, V):
        self.V = V
        self.events = []
        self.cases = []

    @property
    def validators(self):
        return pos.Validators({c + 1: 1 for c in range(self.V)})

    def mk(self, c, sp, others=()):
        """The next event: creator idx c, self-parent sp (None: seq 1)."""
        eid = len(self.events)
        parents = ([sp.id] if sp is not None else []) + [o.id for o in others]
        lam = 1 + max([self.events[p].lamport for p in parents], default=0)
        e = Event(eid, c + 1, sp.seq + 1 if sp is not None else 1, lam, parents, "e%d" % eid)
        self.events.append(e)
        return e

    def chain(self, c, sp, n):
        """n more events of c on top of sp, no other parents."""
        out = []
        for _ in range(n):
            sp = self.mk(c, sp)
            out.append(sp)
        return out

    def case(self, head, want, creator=0):
        self.cases.append((head.id, creator, tuple(getattr(v, "id", v) for v in want)))


def twin():
    """A second child of one self-parent."""
    d = Dag(4)
    a1 = d.mk(0, None)
    a2 = d.mk(0, a1)
    t2 = d.mk(0, a1)                                         # the twin of a2
    b1 = d.mk(1, None, [a2])
    c1 = d.mk(2, None, [t2])
    d1 = d.mk(3, None, [b1, c1])
    t3 = d.mk(0, t2, [b1])                                   # on the twin's branch, sees a2 through b1
    d.case(b1, NO_EVIDENCE)                                  # only the first twin
    d.case(c1, NO_EVIDENCE)                                  # only the second
    d.case(d1, (a2, t2, 2))                                  # both
    d.case(t2, NO_EVIDENCE)                                  # the second twin itself: a1 and itself
    d.case(a2, NO_EVIDENCE)
    d.case(t3, (a2, t2, 2))
    d.case(d1, NO_EVIDENCE, creator=1)                       # an honest creator
    return d


def twin_self():
    """The head is itself the second twin and sees the first through another
    creator."""
    d = Dag(3)
    a1 = d.mk(0, None)
    a2 = d.mk(0, a1)
    b1 = d.mk(1, None, [a2])
    t2 = d.mk(0, a1, [b1])
    d.case(t2, (a2, t2, 2))
    d.case(b1, NO_EVIDENCE)
    return d


def twin_roots():
    """Two seq-1 events of one creator."""
    d = Dag(3)
    a1 = d.mk(0, None)
    r1 = d.mk(0, None)
    b1 = d.mk(1, None, [a1])
    c1 = d.mk(2, None, [r1])
    b2 = d.mk(1, b1, [c1])
    r2 = d.mk(0, r1)
    c2 = d.mk(2, c1, [r2])
    d.case(b1, NO_EVIDENCE)
    d.case(c1, NO_EVIDENCE)
    d.case(c2, NO_EVIDENCE)                                  # r1, r2: one branch
    d.case(b2, (a1, r1, 1))
    return d


def triple():
    """Three children of one self-parent: the two lowest of those observed."""
    d = Dag(3)
    a1 = d.mk(0, None)
    a2 = d.mk(0, a1)
    t2 = d.mk(0, a1)
    u2 = d.mk(0, a1)
    b1 = d.mk(1, None, [u2])
    c1 = d.mk(2, None, [t2])
    c2 = d.mk(2, c1, [b1])                                   # t2 and u2
    b2 = d.mk(1, b1, [a2])                                   # a2 and u2
    b3 = d.mk(1, b2, [c2])                                   # all three
    d.case(b1, NO_EVIDENCE)
    d.case(c2, (t2, u2, 2))
    d.case(b2, (a2, u2, 2))
    d.case(b3, (a2, t2, 2))
    return d


def nested():
    """Branch b1 forks off b0 at seq 3, b2 forks off b1 at seq 5."""
    d = Dag(4)
    b0 = d.chain(0, None, 6)                                 # seqs 1..6
    b1 = d.chain(0, b0[1], 4)                                # seqs 3..6 on top of seq 2
    b2 = d.chain(0, b1[1], 2)                                # seqs 5..6 on top of b1's seq 4
    p = d.mk(1, None, [b2[-1]])                              # b2's tip: b0 to seq 2, b1 to seq 4, b2
    q = d.mk(2, None, [b0[3]])                               # b0 to seq 4
    h1 = d.mk(1, p, [q])
    s = d.mk(3, None, [b1[-1]])                              # b1 to seq 6 (b0 to seq 2)
    h3 = d.mk(3, s, [p])
    d.case(h1, (b0[2], b1[0], 3))
    d.case(p, NO_EVIDENCE)                                   # the three intervals [1,2] [3,4] [5,6] are disjoint
    d.case(q, NO_EVIDENCE)
    d.case(s, NO_EVIDENCE)
    d.case(h3, (b1[2], b2[0], 5))
    return d


MANY = 70


def many():
    """One creator with 70 branches: 69 more children of its first event,
    every third of them with a child of its own."""
    d = Dag(3)
    a1 = d.mk(0, None)
    kids = [d.mk(0, a1) for _ in range(MANY)]                # kids[0] stays on the original branch
    tips = [d.mk(0, k) if j % 3 == 0 else k for j, k in enumerate(kids)]
    bs = []
    for t in tips:                                           # creator 1 collects them one by one
        bs.append(d.mk(1, bs[-1] if bs else None, [t]))
    b = bs[-1]
    c1 = d.mk(2, None, [tips[65]])
    c2 = d.mk(2, c1, [tips[68]])                             # the branches at places 65 and 68 of the creator's list
    c3 = d.mk(2, c2, [tips[66]])                             # and 66, which holds two events
    d.case(b, (kids[0], kids[1], 2))
    d.case(c1, NO_EVIDENCE)
    d.case(c2, (kids[65], kids[68], 2))
    d.case(c3, (kids[65], kids[66], 2))
    d.case(bs[0], NO_EVIDENCE)
    d.case(bs[2], (kids[0], kids[1], 2))                     # the first three branches
    return d


def long_chain():
    """300 events of one creator, the fork at seq 257: the branch -> event
    table grows past its first 256 seqs, the search runs nine steps deep."""
    d = Dag(3)
    a = d.chain(0, None, 300)
    f = d.chain(0, a[255], 2)                                # seqs 257, 258 on top of seq 256
    b1 = d.mk(1, None, [a[-1]])
    c1 = d.mk(2, None, [f[-1]])
    b2 = d.mk(1, b1, [c1])
    c2 = d.mk(2, c1, [a[256]])                               # the original branch up to seq 257 exactly
    d.case(b1, NO_EVIDENCE)
    d.case(c1, NO_EVIDENCE)
    d.case(b2, (a[256], f[0], 257))
    d.case(c2, (a[256], f[0], 257))
    return d


DAGS = {"twin": twin, "twin_self": twin_self, "twin_roots": twin_roots, "triple": triple, "nested": nested,
        "many": many, "long": long_chain}
