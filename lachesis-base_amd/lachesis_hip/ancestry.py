"""Ancestry from the vector clock over include/lachesis_ancestry.h.

The reference finds the events a block confirms with a DFS over the parent
lists (``Engine.DfsSubgraph``, vecengine/traversal.go:10-37; the same walk is
``Lachesis.confirmEvents``, abft/lachesis.go:40-55).  The index holds the
answer: "x is an ancestor of a" is one HighestBefore entry of a (one
LowestAfter entry of x where a sees x's creator as a cheater), so the set is a
scan over the epoch's events on the device
(lachesis-base_amd/csrc/lx_ancestry.{cpp,hip}).  :class:`AncestryIndex` keeps
one label per event, e.g. the frame that confirmed it.

Fork evidence: where a head sees a creator as a cheater, ``fork_pairs`` /
``cheaters`` name the two events that prove it -- the two lowest events of that
creator, at the lowest seq, that share a seq and are both observed by the head.

Like :class:`lachesis_hip.mediantime.MedianTimeIndex` this module only keeps
the event-ID -> dense-index map of the :class:`VecfcIndex` it is built on.
"""

import ctypes

import numpy as np

from .capi import LxError, _p, u8p, u32p, vp

NONE = 0xFFFFFFFF   # LX_ANC_NONE: no event


class AncestryIndex:
    """``dagi`` is a :class:`lachesis_hip.VecfcIndex` (unsharded).  The handle
    follows the index's ``reset`` / ``drop_not_flushed`` / ``restore`` by
    itself: afterwards it holds no label of an event whose dense index was
    given up."""

    def __init__(self, dagi):
        self.dagi = dagi
        self.L = dagi.ix.L
        h = vp()
        rc = self.L.lx_anc_create(dagi.ix.h, ctypes.byref(h))
        if rc != 0:
            raise LxError(rc, self.L.lx_last_error(dagi.ix.h).decode() or "lx_anc_create failed")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.lx_anc_destroy(self.h)
            self.h = None

    __del__ = close

    def _chk(self, rc):
        if rc != 0:
            raise LxError(rc, self.L.lx_anc_last_error(self.h).decode())

    def reset(self):
        """No labels held (also noticed without this call after a new epoch)."""
        self._chk(self.L.lx_anc_reset(self.h))

    def _dense(self, ids):
        out = np.empty(len(ids), dtype=np.uint32)
        for k, eid in enumerate(ids):
            i = self.dagi._idx(getattr(eid, "id", eid))
            if i is None:
                raise LxError(-2, "event %r not indexed" % (eid,))
            out[k] = i
        return out

    # dense indices -----------------------------------------------------------
    def observes_dense(self, head, x):
        """lx_anc_observes: ``out[i]`` = x[i] is head[i] or an ancestor of it."""
        head = np.ascontiguousarray(head, dtype=np.uint32)
        x = np.ascontiguousarray(x, dtype=np.uint32)
        if len(head) != len(x):
            raise ValueError("one x per head")
        out = np.zeros(len(head), dtype=np.uint8)
        if len(head):
            self._chk(self.L.lx_anc_observes(self.h, len(head), _p(head, u32p), _p(x, u32p), _p(out, u8p)))
        return out.astype(bool)

    def confirm_dense(self, heads, labels):
        """lx_anc_confirm: the events each head labelled, one ascending array of
        dense indices per head in call order."""
        heads = np.ascontiguousarray(heads, dtype=np.uint32)
        labels = np.ascontiguousarray(labels, dtype=np.uint32)
        if len(heads) != len(labels):
            raise ValueError("one label per head")
        n_new = np.zeros(max(len(heads), 1), dtype=np.uint32)
        self._chk(self.L.lx_anc_confirm(self.h, len(heads), _p(heads, u32p), _p(labels, u32p), _p(n_new, u32p)))
        ev = self.last_confirmed_dense()
        cuts = np.cumsum(n_new[:len(heads)], dtype=np.uint64)
        assert (int(cuts[-1]) if len(cuts) else 0) == len(ev)
        return [ev[int(a):int(b)] for a, b in zip([0] + list(cuts[:-1]), cuts)]

    def last_confirmed_dense(self):
        n = ctypes.c_uint64()
        self._chk(self.L.lx_anc_last_confirmed(self.h, None, 0, ctypes.byref(n)))
        out = np.zeros(max(n.value, 1), dtype=np.uint32)
        self._chk(self.L.lx_anc_last_confirmed(self.h, _p(out, u32p), n.value, ctypes.byref(n)))
        return out[:n.value]

    def labels_dense(self, first=0, n=None):
        """lx_anc_labels of events [first, first + n) (default: to the last)."""
        if n is None:
            n = len(self.dagi.ids) - first
        out = np.zeros(max(n, 1), dtype=np.uint32)
        self._chk(self.L.lx_anc_labels(self.h, int(first), int(n), _p(out, u32p)))
        return out[:n]

    def set_labels_dense(self, first, labels):
        lab = np.ascontiguousarray(labels, dtype=np.uint32)
        self._chk(self.L.lx_anc_set_labels(self.h, int(first), len(lab), _p(lab, u32p)))

    def low_water(self):
        """The lowest dense index without a label."""
        ev = ctypes.c_uint64()
        self._chk(self.L.lx_anc_low_water(self.h, ctypes.byref(ev)))
        return ev.value

    def fork_pairs_dense(self, heads, creators):
        """lx_anc_fork_pairs: arrays ``(x, y, seq)``, pairwise for (heads[i],
        creators[i]); ``x < y`` the canonical pair of events of that creator
        (validator idx) with equal seq that the head observes, or
        ``(NONE, NONE, 0)``."""
        heads = np.ascontiguousarray(heads, dtype=np.uint32)
        creators = np.ascontiguousarray(creators, dtype=np.uint32)
        if len(heads) != len(creators):
            raise ValueError("one creator per head")
        n = len(heads)
        x, y, seq = (np.zeros(max(n, 1), dtype=np.uint32) for _ in range(3))
        if n:
            self._chk(self.L.lx_anc_fork_pairs(self.h, n, _p(heads, u32p), _p(creators, u32p), _p(x, u32p),
                                               _p(y, u32p), _p(seq, u32p)))
        return x[:n], y[:n], seq[:n]

    def last_cheaters_dense(self):
        """The list of the last lx_anc_cheaters: arrays (creator, x, y, seq)."""
        n = ctypes.c_uint64()
        self._chk(self.L.lx_anc_last_cheaters(self.h, None, None, None, None, 0, ctypes.byref(n)))
        c, x, y, s = (np.zeros(max(n.value, 1), dtype=np.uint32) for _ in range(4))
        self._chk(self.L.lx_anc_last_cheaters(self.h, _p(c, u32p), _p(x, u32p), _p(y, u32p), _p(s, u32p), n.value,
                                              ctypes.byref(n)))
        return c[:n.value], x[:n.value], y[:n.value], s[:n.value]

    def cheaters_dense(self, heads):
        """lx_anc_cheaters: per head, in call order, the list of ``(creator, x,
        y, seq)`` of every cheater it observes, ascending creator idx."""
        heads = np.ascontiguousarray(heads, dtype=np.uint32)
        n_found = np.zeros(max(len(heads), 1), dtype=np.uint32)
        self._chk(self.L.lx_anc_cheaters(self.h, len(heads), _p(heads, u32p), _p(n_found, u32p)))
        c, x, y, s = self.last_cheaters_dense()
        cuts = np.cumsum(n_found[:len(heads)], dtype=np.uint64)
        assert (int(cuts[-1]) if len(cuts) else 0) == len(c)
        rows = list(zip((int(v) for v in c), (int(v) for v in x), (int(v) for v in y), (int(v) for v in s)))
        return [rows[int(a):int(b)] for a, b in zip([0] + list(cuts[:-1]), cuts)]

    # event IDs ---------------------------------------------------------------
    def observes(self, heads, xs):
        """``heads`` / ``xs``: events or their IDs, pairwise."""
        return self.observes_dense(self._dense(heads), self._dense(xs))

    def confirm(self, heads, labels):
        """confirmEvents of ``heads`` (events or IDs) in call order: per head
        the list of event IDs it labelled (a set: ascending Add order, not the
        reference's DFS order)."""
        ids = self.dagi.ids
        return [[ids[int(i)] for i in g] for g in self.confirm_dense(self._dense(heads), labels)]

    def labels(self, ids):
        """GetEventConfirmedOn of every event (or ID) in ``ids``; 0 = none."""
        all_ = self.labels_dense()
        return all_[self._dense(ids)] if len(ids) else all_[:0]

    def set_labels(self, ids, labels):
        """Labels of events by ID (a restart: the stored confirmed-on table)."""
        at = dict(zip((int(i) for i in self._dense(ids)), (int(l) for l in labels)))
        idx = sorted(at)
        lo = 0
        while lo < len(idx):
            hi = lo + 1
            while hi < len(idx) and idx[hi] == idx[hi - 1] + 1:
                hi += 1
            self.set_labels_dense(idx[lo], [at[i] for i in idx[lo:hi]])
            lo = hi

    def fork_pairs(self, heads, creators):
        """``heads``: events or IDs, ``creators``: validator idxs, pairwise.
        Per pair ``(event ID, event ID, seq)`` or ``None``."""
        ids = self.dagi.ids
        x, y, seq = self.fork_pairs_dense(self._dense(heads), creators)
        return [None if int(a) == NONE else (ids[int(a)], ids[int(b)], int(s)) for a, b, s in zip(x, y, seq)]

    def cheaters(self, heads):
        """Per head (event or ID) the list of ``(creator idx, event ID, event
        ID, seq)`` of every cheater it observes."""
        ids = self.dagi.ids
        return [[(c, ids[a], ids[b], s) for c, a, b, s in g] for g in self.cheaters_dense(self._dense(heads))]
