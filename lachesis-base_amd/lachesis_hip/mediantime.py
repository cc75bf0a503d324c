"""vecmt's MedianTime over include/lachesis_mediantime.h.

The production consumers of lachesis-base carry every event's creation time
beside HighestBeforeSeq (the reference's vecengine is generic over its vectors
for this, vecengine/vector.go:8-22) and take the stake-weighted median of the
creation times of the highest events an Atropos observes as the block's time.
:class:`MedianTimeIndex` gives that value, and the merged HighestBeforeTime
vector it is taken over, from the GPU index: the caller hands over each
event's creation time once, the device derives everything else from the
HighestBefore plane (lachesis-base_amd/csrc/lx_mediantime.{cpp,hip}).

Like :class:`lachesis_hip.emitter.QuorumIndexer` this module only keeps the
event-ID -> dense-index map of the :class:`VecfcIndex` it is built on.
"""

import ctypes

import numpy as np

from .capi import LxError, _p, u32p, u64p, vp


class MedianTimeIndex:
    """``dagi`` is a :class:`lachesis_hip.VecfcIndex` (unsharded).  The handle
    follows the index's ``reset`` / ``drop_not_flushed`` / ``restore`` by
    itself: afterwards it holds no time of an event whose dense index was given
    up."""

    def __init__(self, dagi):
        self.dagi = dagi
        self.L = dagi.ix.L
        h = vp()
        rc = self.L.lx_mt_create(dagi.ix.h, ctypes.byref(h))
        if rc != 0:
            raise LxError(rc, self.L.lx_last_error(dagi.ix.h).decode() or "lx_mt_create failed")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.lx_mt_destroy(self.h)
            self.h = None

    __del__ = close

    def _chk(self, rc):
        if rc != 0:
            raise LxError(rc, self.L.lx_mt_last_error(self.h).decode())

    def reset(self):
        """New epoch: no times held (also noticed without this call)."""
        self._chk(self.L.lx_mt_reset(self.h))

    def num_times(self):
        return int(self.L.lx_mt_num_times(self.h))

    def set_times_dense(self, first_event, times):
        """lx_mt_set_times: creation times of the dense events
        [first_event, first_event + len(times))."""
        t = np.ascontiguousarray(times, dtype=np.uint64)
        self._chk(self.L.lx_mt_set_times(self.h, int(first_event), len(t), _p(t, u64p)))

    def set_times(self, events, times):
        """Creation times of ``events`` (events or their IDs).  Events the
        index does not hold yet are taken to be added next, in the order given
        (times may be handed over before ``add_events``)."""
        nxt = len(self.dagi.ids)
        at = {}
        for e, t in zip(events, times):
            eid = getattr(e, "id", e)
            i = self.dagi._idx(eid)
            if i is None:
                i, nxt = nxt, nxt + 1
            at[i] = int(t)
        idx = sorted(at)
        lo = 0
        while lo < len(idx):
            hi = lo + 1
            while hi < len(idx) and idx[hi] == idx[hi - 1] + 1:
                hi += 1
            self.set_times_dense(idx[lo], [at[i] for i in idx[lo:hi]])
            lo = hi

    def _dense(self, ids):
        out = np.empty(len(ids), dtype=np.uint32)
        for k, eid in enumerate(ids):
            i = self.dagi._idx(eid)
            if i is None:
                raise LxError(-2, "event %r not indexed" % (eid,))
            out[k] = i
        return out

    def median_time_dense(self, ev, default_time):
        ev = np.ascontiguousarray(ev, dtype=np.uint32)
        out = np.zeros(len(ev), dtype=np.uint64)
        if len(ev):
            self._chk(self.L.lx_mt_median_time(self.h, len(ev), _p(ev, u32p), int(default_time), _p(out, u64p)))
        return out

    def merged_times_dense(self, ev):
        ev = np.ascontiguousarray(ev, dtype=np.uint32)
        V = len(self.dagi.validators.weights)
        out = np.zeros(len(ev) * V, dtype=np.uint64)
        if len(ev):
            self._chk(self.L.lx_mt_merged_times(self.h, len(ev), _p(ev, u32p), _p(out, u64p)))
        return out.reshape(len(ev), V)

    def median_time(self, ids, default_time):
        """MedianTime(id, default_time) of every event ID in ``ids`` (uint64 array)."""
        return self.median_time_dense(self._dense(ids), default_time)

    def merged_times(self, ids):
        """Merged HighestBeforeTime rows, ``len(ids)`` x V (0: fork-detected or unobserved)."""
        return self.merged_times_dense(self._dense(ids))
