"""abft.IndexedLachesis over the HIP library (include/lachesis_abft.h).

Mirrors the reference's consensus surface so the parity tests drive it like
abft/common_test.go drives FakeLachesis:

* ``IndexedLachesis(validators, epoch)``   -- NewIndexedLachesis + ApplyGenesis
  (abft/indexed_lachesis.go:42-51, abft/apply_genesis.go:17-44)
* ``bootstrap(begin_block)``               -- Bootstrap with
  lachesis.ConsensusCallbacks: ``begin_block(block) -> (apply_event, end_block)``
  (lachesis/consensus.go:21-44); ``end_block()`` returns the next epoch's
  validators to seal the epoch, or None
* ``build(e)`` / ``process(e)``            -- Build / Process
  (abft/indexed_lachesis.go:53-82); ``process_batch(events)`` processes many
  events in one call with the same results
* ``build_frames(events)``                 -- Build for candidate events that are
  not added (lx_abft_build_frames): sets ``e.frame``, returns the is-root
  flags; no Add, no rollback
* ``build_progress(events)`` / ``event_progress(events)`` -- how far candidate
  or processed events are from the next frame (lx_abft_build_progress,
  lx_abft_event_progress); ``progress_pairs()`` reads the per-root stakes
* ``reset(epoch, validators)``             -- Orderer.Reset (abft/bootstrap.go:54-65)
* ``state()`` / ``restore(state, index_db, get_event, begin_block)`` -- the
  abft state a caller persists, and Bootstrap over it after a restart
  (abft/bootstrap.go:34-55 over a non-empty Store; lx_abft_state_fetch,
  lx_abft_restore) instead of replaying the epoch
* ``store``                                -- the bits of abft.Store the tests read
  (GetEpoch, GetValidators, GetLastDecidedFrame, GetFrameRoots,
  GetEventConfirmedOn)

``validators`` is any object with ``ids`` (idx order), ``weights`` (idx
order) and ``idxs`` (ID -> idx), like pos.Validators.  Events carry ``id``,
``creator``, ``seq``, ``parents`` (ids, self-parent first) and ``frame``.
All computation is on the GPU; there is no CPU path.
"""

import ctypes

import numpy as np

from .capi import Index, LxError, _p, u32p, u64p, vp

FRAME_BUILD = 0xFFFFFFFF
ERR_FRAME = -7
ERR_BYZANTINE = -8


class Block:
    """lachesis.Block {Atropos, Cheaters} (lachesis/block.go)."""

    def __init__(self, atropos, cheaters):
        self.atropos = atropos
        self.cheaters = cheaters

    def __eq__(self, o):
        return (self.atropos, self.cheaters) == (o.atropos, o.cheaters)

    def __repr__(self):
        return "Block(%r, cheaters=%r)" % (self.atropos, self.cheaters)


class WrongFrameError(RuntimeError):
    """ErrWrongFrame (abft/event_processing.go:11-13)."""


class _Validators:
    """Minimal pos.Validators built from weights by ID (sorted as
    inter/pos/sort.go:16-22) for validator sets returned by end_block."""

    def __init__(self, ids, weights):
        self.ids = list(ids)
        self.weights = list(weights)
        self.idxs = {v: i for i, v in enumerate(self.ids)}


BEGIN_BLOCK = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32,
                               ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint32)
APPLY_EVENT = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_uint32)
END_BLOCK = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32),
                             ctypes.POINTER(ctypes.POINTER(ctypes.c_uint32)))


class Callbacks(ctypes.Structure):
    _fields_ = [("user", ctypes.c_void_p), ("begin_block", BEGIN_BLOCK), ("apply_event", APPLY_EVENT),
                ("end_block", END_BLOCK)]


class AbftStats(ctypes.Structure):
    _fields_ = [("ms_index", ctypes.c_float), ("ms_frames", ctypes.c_float), ("ms_election", ctypes.c_float),
                ("ms_blocks", ctypes.c_float), ("frame_steps", ctypes.c_uint32), ("fc_launches", ctypes.c_uint32),
                ("vote_launches", ctypes.c_uint32), ("blocks", ctypes.c_uint32), ("fc_pairs", ctypes.c_uint64),
                ("fc_pair_cols", ctypes.c_uint64), ("ms_root_fc_gpu", ctypes.c_float),
                ("fc_lane_ops", ctypes.c_uint64), ("elections_ahead", ctypes.c_uint32)]


class BuildStats(ctypes.Structure):
    """lx_abft_build_stats."""
    _fields_ = [("launches", ctypes.c_uint32), ("frame_steps", ctypes.c_uint32), ("rounds", ctypes.c_uint32),
                ("fc16", ctypes.c_uint32), ("fc_pairs", ctypes.c_uint64)]


def build_frames_arrays(L, h, creator, seq, poff, par, chk=None):
    """lx_abft_build_frames on dense arrays: (frames, is_root).  Without
    ``chk`` returns (rc, err_index, frames, is_root) instead of raising."""
    creator = np.ascontiguousarray(creator, dtype=np.uint32)
    seq = np.ascontiguousarray(seq, dtype=np.uint32)
    poff = np.ascontiguousarray(poff, dtype=np.uint64)
    par = np.ascontiguousarray(par if len(par) else [0], dtype=np.uint32)
    n = len(creator)
    frames = np.zeros(max(n, 1), dtype=np.uint32)
    roots = np.zeros(max(n, 1), dtype=np.uint8)
    err = ctypes.c_uint32()
    rc = L.lx_abft_build_frames(h, n, _p(creator, u32p), _p(seq, u32p), _p(poff, u64p), _p(par, u32p),
                                _p(frames, u32p), roots.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                ctypes.byref(err))
    if chk is None:
        return rc, err.value, frames[:n], roots[:n]
    if rc != 0:
        ex = LxError(rc, L.lx_abft_last_error(h).decode())
        ex.err_index = err.value
        raise ex
    return frames[:n], roots[:n]


PROGRESS_PAIRS = 1
PROGRESS_FIELDS = ("frame", "n_roots", "n_caused", "stake", "root_stake")


def _progress_out(n):
    out = {f: np.zeros(max(n, 1), dtype=np.uint64 if f == "root_stake" else np.uint32) for f in PROGRESS_FIELDS}
    ptrs = [_p(out[f], u64p if f == "root_stake" else u32p) for f in PROGRESS_FIELDS]
    return out, ptrs


def _progress_done(L, h, rc, err, out, n, chk):
    res = {f: v[:n] for f, v in out.items()}
    if chk is None:
        return rc, err.value, res
    if rc != 0:
        ex = LxError(rc, L.lx_abft_last_error(h).decode())
        ex.err_index = err.value
        raise ex
    return res


def build_progress_arrays(L, h, creator, seq, poff, par, at_frame=None, pairs=False, chk=None, flags=None):
    """lx_abft_build_progress on dense arrays: a dict of arrays ``frame``,
    ``n_roots``, ``n_caused``, ``stake``, ``root_stake`` per candidate.
    ``at_frame``: per candidate FRAME_BUILD or the frame to ask (None: Build
    frames).  ``pairs`` keeps the pair stakes for :func:`progress_pairs`.
    Without ``chk`` returns (rc, err_index, dict) instead of raising."""
    creator = np.ascontiguousarray(creator, dtype=np.uint32)
    seq = np.ascontiguousarray(seq, dtype=np.uint32)
    poff = np.ascontiguousarray(poff, dtype=np.uint64)
    par = np.ascontiguousarray(par if len(par) else [0], dtype=np.uint32)
    n = len(creator)
    at = None if at_frame is None else np.ascontiguousarray(at_frame if n else [0], dtype=np.uint32)
    out, ptrs = _progress_out(n)
    err = ctypes.c_uint32()
    fl = (PROGRESS_PAIRS if pairs else 0) if flags is None else int(flags)
    rc = L.lx_abft_build_progress(h, n, _p(creator, u32p), _p(seq, u32p), _p(poff, u64p), _p(par, u32p),
                                  None if at is None else _p(at, u32p), fl, *ptrs, ctypes.byref(err))
    return _progress_done(L, h, rc, err, out, n, chk)


def event_progress_arrays(L, h, events, at_frame=None, pairs=False, chk=None, flags=None):
    """lx_abft_event_progress: the same for indexed events (dense indices)."""
    n = len(events)
    ev = np.ascontiguousarray(events if n else [0], dtype=np.uint32)
    at = None if at_frame is None else np.ascontiguousarray(at_frame if n else [0], dtype=np.uint32)
    out, ptrs = _progress_out(n)
    err = ctypes.c_uint32()
    fl = (PROGRESS_PAIRS if pairs else 0) if flags is None else int(flags)
    rc = L.lx_abft_event_progress(h, n, _p(ev, u32p), None if at is None else _p(at, u32p), fl, *ptrs,
                                  ctypes.byref(err))
    return _progress_done(L, h, rc, err, out, n, chk)


def progress_pairs(L, h, n, cap=None):
    """lx_abft_last_progress_pairs after a progress call of ``n`` entries made
    with ``pairs``: (pair_off[n + 1], root events, stakes, n_pairs).  ``cap``
    limits the entries written (None: all); n_pairs is the full count.  After
    any other call on the handle the reader is empty: pass n = 0."""
    total = ctypes.c_uint64()
    off = np.zeros(n + 1, dtype=np.uint64)
    rc = L.lx_abft_last_progress_pairs(h, _p(off, u64p), None, None, 0, ctypes.byref(total))
    if rc != 0:
        raise LxError(rc, L.lx_abft_last_error(h).decode())
    want = total.value if cap is None else min(int(cap), total.value)
    root = np.zeros(max(want, 1), dtype=np.uint32)
    stake = np.zeros(max(want, 1), dtype=np.uint32)
    rc = L.lx_abft_last_progress_pairs(h, _p(off, u64p), _p(root, u32p), _p(stake, u32p), want, ctypes.byref(total))
    if rc != 0:
        raise LxError(rc, L.lx_abft_last_error(h).decode())
    return off, root[:want], stake[:want], total.value


class AbftState(ctypes.Structure):
    _fields_ = [("epoch", ctypes.c_uint32), ("last_decided_frame", ctypes.c_uint32), ("n_events", ctypes.c_uint32),
                ("n_frames", ctypes.c_uint32), ("n_slots", ctypes.c_uint64)]


def _fetch_state(L, h, chk):
    """lx_abft_state_sizes + lx_abft_state_fetch: the abft state of the
    current epoch on dense event indices."""
    st = AbftState()
    chk(L.lx_abft_state_sizes(h, ctypes.byref(st)))
    ev_frame = np.zeros(max(st.n_events, 1), dtype=np.uint32)
    ev_conf = np.zeros(max(st.n_events, 1), dtype=np.uint32)
    root_off = np.zeros(st.n_frames + 1, dtype=np.uint64)
    root_ev = np.zeros(max(st.n_slots, 1), dtype=np.uint32)
    chk(L.lx_abft_state_fetch(h, _p(ev_frame, u32p), _p(ev_conf, u32p), _p(root_off, u64p), _p(root_ev, u32p)))
    return dict(epoch=st.epoch, last_decided_frame=st.last_decided_frame, ev_frame=ev_frame[:st.n_events],
                ev_confirmed_on=ev_conf[:st.n_events], root_off=root_off, root_ev=root_ev[:st.n_slots])


def restore_arrays(L, h, state, weights, creator, seq, poff, par, cb):
    """lx_abft_restore on a handle whose index was reloaded: ``state`` as
    ``state()`` returns it, the events as given to lx_load_rows.  Returns the
    library's return code (the message stays in lx_abft_last_error)."""
    w = np.ascontiguousarray(weights, dtype=np.uint32)
    creator = np.ascontiguousarray(creator, dtype=np.uint32)
    seq = np.ascontiguousarray(seq, dtype=np.uint32)
    poff = np.ascontiguousarray(poff, dtype=np.uint64)
    par = np.ascontiguousarray(par if len(par) else [0], dtype=np.uint32)
    ev_frame = np.ascontiguousarray(state["ev_frame"], dtype=np.uint32)
    ev_conf = np.ascontiguousarray(state["ev_confirmed_on"], dtype=np.uint32)
    root_off = np.ascontiguousarray(state["root_off"], dtype=np.uint64)
    root_ev = np.ascontiguousarray(state["root_ev"] if len(state["root_ev"]) else [0], dtype=np.uint32)
    if len(creator) != len(ev_frame) or len(ev_conf) != len(ev_frame) or len(poff) != len(creator) + 1:
        raise ValueError("abft state and event arrays differ in length")
    return L.lx_abft_restore(h, int(state["epoch"]), len(w), _p(w, u32p), int(state["last_decided_frame"]),
                             len(ev_frame), _p(creator, u32p), _p(seq, u32p), _p(poff, u64p), _p(par, u32p),
                             _p(ev_frame, u32p), _p(ev_conf, u32p), len(root_off) - 1, _p(root_off, u64p),
                             _p(root_ev, u32p), None if cb is None else ctypes.byref(cb))


class _StoreView:
    def __init__(self, lch):
        self._l = lch

    def get_epoch(self):
        return self._l.L.lx_abft_epoch(self._l.h)

    def get_validators(self):
        return self._l.validators

    @property
    def last_decided_frame(self):
        return self._l.L.lx_abft_last_decided_frame(self._l.h)

    def get_frame_roots(self, f):
        """Root event ids of frame f (abft/store_roots.go:52-93)."""
        n = ctypes.c_uint32()
        self._l._chk(self._l.L.lx_abft_frame_roots(self._l.h, f, None, 0, ctypes.byref(n)))
        out = np.zeros(max(n.value, 1), dtype=np.uint32)
        self._l._chk(self._l.L.lx_abft_frame_roots(self._l.h, f, _p(out, u32p), n.value, ctypes.byref(n)))
        return [self._l.evs[i].id for i in out[:n.value]]

    def get_event_confirmed_on(self, eid):
        i = self._l.pos.get(eid)
        if i is None:
            return 0
        out = ctypes.c_uint32()
        self._l._chk(self._l.L.lx_abft_event_confirmed_on(self._l.h, i, ctypes.byref(out)))
        return out.value


class IndexedLachesis:
    def __init__(self, validators, epoch=1, device=0, event_capacity=0):
        self.ix = Index(device=device, event_capacity=event_capacity)
        self.L = self.ix.L
        h = vp()
        rc = self.L.lx_abft_create(self.ix.h, ctypes.byref(h))
        if rc != 0:
            raise LxError(rc, "lx_abft_create failed")
        self.h = h
        self.validators = validators
        self.genesis_epoch = epoch
        self.pos = {}
        self.evs = []
        self.store = _StoreView(self)
        self._begin_block = None
        self._cur = None
        self._sealed_with = None
        self._keep = None

    def close(self):
        if getattr(self, "h", None):
            self.L.lx_abft_destroy(self.h)
            self.h = None
        if getattr(self, "ix", None) is not None:
            self.ix.close()

    __del__ = close

    def _chk(self, rc):
        if rc != 0:
            raise LxError(rc, self.L.lx_abft_last_error(self.h).decode())
        return rc

    # callbacks -----------------------------------------------------------------
    def _on_begin(self, user, frame, atropos, cheaters, n):
        block = Block(self.evs[atropos].id, [self.validators.ids[cheaters[k]] for k in range(n)])
        res = self._begin_block(block) if self._begin_block is not None else None
        self._cur = res if res is not None else (None, None)

    def _on_apply(self, user, ev):
        apply_event = self._cur[0] if self._cur else None
        if apply_event is not None:
            apply_event(self.evs[ev])

    def _on_end(self, user, n_out, w_out):
        end_block = self._cur[1] if self._cur else None
        self._cur = None
        nv = end_block() if end_block is not None else None
        if nv is None:
            return 0
        self._sealed_with = nv
        self._seal_w = np.ascontiguousarray(nv.weights, dtype=np.uint32)
        n_out[0] = len(self._seal_w)
        w_out[0] = self._seal_w.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
        return 1

    def bootstrap(self, begin_block=None):
        """Bootstrap (abft/indexed_lachesis.go:84-99, abft/lachesis.go:88-100)."""
        cb = self._callbacks(begin_block)
        w = np.ascontiguousarray(self.validators.weights, dtype=np.uint32)
        self._chk(self.L.lx_abft_bootstrap(self.h, self.genesis_epoch, len(w), _p(w, u32p), ctypes.byref(cb)))

    def _callbacks(self, begin_block):
        self._begin_block = begin_block
        cb = Callbacks(None, BEGIN_BLOCK(self._on_begin) if begin_block is not None else BEGIN_BLOCK(),
                       APPLY_EVENT(self._on_apply), END_BLOCK(self._on_end))
        self._keep = cb
        return cb

    def state(self):
        """The abft state of the current epoch as a caller persists it
        (lx_abft_state_fetch): ``epoch``, ``last_decided_frame``, ``ids`` (event
        ids in dense order), ``ev_frame`` / ``ev_confirmed_on`` per event,
        ``root_off`` / ``root_ev`` (dense indices; frame f = slots
        root_off[f-1] .. root_off[f], in slot order)."""
        st = _fetch_state(self.L, self.h, self._chk)
        st["ids"] = [e.id for e in self.evs]
        return st

    def restore(self, state, index_db, get_event, begin_block=None):
        """Bootstrap over a persisted epoch (abft/indexed_lachesis.go:84-99
        over a non-empty Store, abft/restart_test.go:156-188) on a handle that
        was not bootstrapped, built with the epoch's validators: reloads the
        index from ``index_db`` (tables "S" / "s" / "b" keyed by event id and
        "B", as :meth:`VecfcIndex.flush` writes them) in the dense order of
        ``state["ids"]``, then lx_abft_restore.  Frames decided during the
        call fire no callbacks (lachesis.go:92-98)."""
        from .vecfc import load_epoch_tables
        ids = list(state["ids"])
        self.ix.reset(self.validators.weights)
        load_epoch_tables(self.ix, self.validators, index_db, get_event, order=ids)
        evs = [get_event(i) for i in ids]
        self.pos, self.evs = {}, []
        creator, seq, off, flat = self._dense(evs)
        cb = self._callbacks(begin_block)
        rc = restore_arrays(self.L, self.h, state, self.validators.weights, creator, seq, off, flat, cb)
        self._chk(rc)
        self.evs = evs
        self.pos = {e.id: k for k, e in enumerate(evs)}

    def reset(self, epoch, validators):
        """Orderer.Reset (abft/bootstrap.go:54-65)."""
        w = np.ascontiguousarray(validators.weights, dtype=np.uint32)
        self._chk(self.L.lx_abft_reset(self.h, epoch, len(w), _p(w, u32p)))
        self.validators = validators
        self.pos = {}
        self.evs = []

    # events --------------------------------------------------------------------
    def _dense(self, events):
        creator, seq, off, flat = [], [], [0], []
        local = {}
        base = len(self.evs)
        for k, e in enumerate(events):
            creator.append(self.validators.idxs[e.creator])
            seq.append(e.seq)
            for p in e.parents:
                q = self.pos.get(p)
                if q is None:
                    q = local.get(p)
                if q is None:
                    raise KeyError(p)
                flat.append(q)
            off.append(len(flat))
            local[e.id] = base + k
        return (np.array(creator, dtype=np.uint32), np.array(seq, dtype=np.uint32),
                np.array(off, dtype=np.uint64), np.array(flat if flat else [0], dtype=np.uint32))

    def build(self, e):
        """Build (indexed_lachesis.go:53-63): sets e.frame."""
        creator, seq, off, flat = self._dense([e])
        out = ctypes.c_uint32()
        n = int(off[1])
        self._chk(self.L.lx_abft_build(self.h, int(creator[0]), int(seq[0]), n, _p(flat, u32p), ctypes.byref(out)))
        e.frame = out.value

    def build_frames(self, events):
        """Build for candidate events that are not added (lx_abft_build_frames):
        sets ``e.frame`` on each -- what :meth:`build` would set -- and returns
        the is-root flags (frame != selfParentFrame).  Each candidate is judged
        alone; parents are existing events.  Nothing is added or rolled back.
        A refused candidate raises LxError with ``err_index`` = its position."""
        creator = np.array([self.validators.idxs[e.creator] for e in events], dtype=np.uint32)
        seq = np.array([e.seq for e in events], dtype=np.uint32)
        off = np.zeros(len(events) + 1, dtype=np.uint64)
        flat = []
        for k, e in enumerate(events):
            flat.extend(self.pos[p] for p in e.parents)
            off[k + 1] = len(flat)
        frames, roots = build_frames_arrays(self.L, self.h, creator, seq, off, flat, self._chk)
        for e, f in zip(events, frames):
            e.frame = int(f)
        return [bool(r) for r in roots]

    def build_progress(self, events, at_frame=None, pairs=False):
        """Frame progress of candidate events that are not added
        (lx_abft_build_progress): a dict of arrays ``frame``, ``n_roots``,
        ``n_caused``, ``stake``, ``root_stake`` per candidate -- how far each
        is from the next frame.  Nothing is added or rolled back."""
        creator = np.array([self.validators.idxs[e.creator] for e in events], dtype=np.uint32)
        seq = np.array([e.seq for e in events], dtype=np.uint32)
        off = np.zeros(len(events) + 1, dtype=np.uint64)
        flat = []
        for k, e in enumerate(events):
            flat.extend(self.pos[p] for p in e.parents)
            off[k + 1] = len(flat)
        self._progress_n = len(events)
        return build_progress_arrays(self.L, self.h, creator, seq, off, flat, at_frame, pairs, self._chk)

    def event_progress(self, events, at_frame=None, pairs=False):
        """The same for events already processed (lx_abft_event_progress)."""
        self._progress_n = len(events)
        return event_progress_arrays(self.L, self.h, [self.pos[e.id] for e in events], at_frame, pairs, self._chk)

    def progress_pairs(self, cap=None):
        """Pair stakes of the last progress call made with ``pairs``:
        (pair_off, root event ids, stakes, n_pairs)."""
        off, root, stake, total = progress_pairs(self.L, self.h, getattr(self, "_progress_n", 0), cap)
        return off, [self.evs[r].id for r in root], stake, total

    def build_stats(self):
        """lx_abft_build_last_stats: GPU work of the last :meth:`build_frames`
        or progress call."""
        st = BuildStats()
        self._chk(self.L.lx_abft_build_last_stats(self.h, ctypes.byref(st)))
        return {f: getattr(st, f) for f, _ in BuildStats._fields_}

    def process(self, e):
        """Process (indexed_lachesis.go:65-82): None or the error."""
        consumed, err = self.process_batch([e])
        return err

    def process_batch(self, events, claimed=True):
        """Processes events in order; returns (consumed, error).  ``claimed``
        False trusts the computed frames (Build then Process).  consumed <
        len(events) without error means a block sealed the epoch."""
        events = list(events)
        if not events:
            return 0, None
        try:
            creator, seq, off, flat = self._dense(events)
        except KeyError as k:
            # Add fails for an unknown parent (vecengine/index.go:159-161):
            # process the events before the first such event
            bad = next(i for i, e in enumerate(events)
                       if any(p not in self.pos and p not in {x.id for x in events[:i]} for p in e.parents))
            c, err = self.process_batch(events[:bad], claimed) if bad else (0, None)
            if err is not None or c < bad:
                return c, err
            return c, LxError(-2, "processed out of order, parent not found (inconsistent DB), parent=%r" % (k.args[0],))
        frames = np.array([e.frame if claimed else FRAME_BUILD for e in events], dtype=np.uint32)
        out = np.zeros(len(events), dtype=np.uint32)
        consumed = ctypes.c_uint32()
        base = len(self.evs)
        for k, e in enumerate(events):
            self.pos[e.id] = base + k
            self.evs.append(e)
        epoch0 = self.store.get_epoch()
        self._sealed_with = None
        rc = self.L.lx_abft_process_batch(self.h, len(events), _p(creator, u32p), _p(seq, u32p), _p(off, u64p),
                                          _p(flat, u32p), _p(frames, u32p), _p(out, u32p), ctypes.byref(consumed))
        c = consumed.value
        if not claimed:
            for k in range(c):
                events[k].frame = int(out[k])
        if self.store.get_epoch() != epoch0:
            # sealed: a new, empty epoch (frame_decide.go:52-58)
            self.validators = self._sealed_with
            self.pos = {}
            self.evs = []
        else:
            for e in events[c:]:
                del self.pos[e.id]
            del self.evs[base + c:]
        if rc == ERR_FRAME:
            return c, WrongFrameError("claimed frame mismatched with calculated")
        if rc != 0:
            raise LxError(rc, self.L.lx_abft_last_error(self.h).decode())
        return c, None

    def frame_of(self, eid):
        out = ctypes.c_uint32()
        self._chk(self.L.lx_abft_event_frame(self.h, self.pos[eid], ctypes.byref(out)))
        return out.value

    def last_stats(self):
        st = AbftStats()
        self._chk(self.L.lx_abft_last_stats(self.h, ctypes.byref(st)))
        return {f: getattr(st, f) for f, _ in AbftStats._fields_}

    def set_option(self, name, value):
        """lx_abft_set_option (path selection; results never change)."""
        self._chk(self.L.lx_abft_set_option(self.h, name.encode(), int(value)))


class DenseLachesis:
    """Dense-index handle over lx_abft_* (what a cgo shim binds 1:1): events
    are Add-order indices of the current epoch, validators are idx-ordered
    weights.  Records blocks as (epoch, frame, atropos, cheaters, confirmed);
    ``apply_events=False`` skips the per-event ApplyEvent callback (the
    confirmation DFS still runs; GetEventConfirmedOn still answers).
    ``seal(epoch, frame)`` may return the next epoch's weights.
    ``block_log=True``: no callbacks at all -- the library logs each decided
    block itself (option block_log, with the confirmed events when
    apply_events) and the blocks are read after each batch; never seals."""

    def __init__(self, weights, epoch=1, device=0, event_capacity=0, apply_events=True, seal=None, block_log=False,
                 bootstrap=True):
        """``bootstrap=False``: the handle is created but not bootstrapped;
        :meth:`restore` resumes a persisted epoch on it."""
        self.ix = Index(device=device, event_capacity=event_capacity)
        self.L = self.ix.L
        h = vp()
        rc = self.L.lx_abft_create(self.ix.h, ctypes.byref(h))
        if rc != 0:
            raise LxError(rc, "lx_abft_create failed")
        self.h = h
        self.blocks = []
        self.seal = seal
        self._cur = None
        self._seal_w = None
        self.block_log = bool(block_log)
        if self.block_log and seal is not None:
            raise ValueError("block_log never seals: no seal callback")
        self._cb = None if self.block_log else Callbacks(
            None, BEGIN_BLOCK(self._begin), APPLY_EVENT(self._apply) if apply_events else APPLY_EVENT(),
            END_BLOCK(self._end))
        w = np.ascontiguousarray(weights, dtype=np.uint32)
        self.weights = w
        if bootstrap:
            rc = self.L.lx_abft_bootstrap(self.h, epoch, len(w), _p(w, u32p),
                                          None if self._cb is None else ctypes.byref(self._cb))
            if rc != 0:
                raise LxError(rc, self.L.lx_abft_last_error(self.h).decode())
        if self.block_log:
            self.set_option("block_log", 2 if apply_events else 1)

    def _chk(self, rc):
        if rc != 0:
            raise LxError(rc, self.L.lx_abft_last_error(self.h).decode())
        return rc

    def state(self):
        """The abft state of the current epoch on dense indices
        (lx_abft_state_fetch): ``epoch``, ``last_decided_frame``, ``ev_frame``,
        ``ev_confirmed_on``, ``root_off``, ``root_ev``."""
        return _fetch_state(self.L, self.h, self._chk)

    def restore(self, state, creator, seq, poff, par, tables, chunk=4096):
        """Resumes a persisted epoch on a handle created with
        ``bootstrap=False``: reloads the index from ``tables`` -- what
        :meth:`Index.writeback` returned at the epoch's flushes, merged:
        {"S" / "s" / "b": {dense index: bytes}, "B": RLP(BranchesInfo)} -- for
        the events given as to lx_add_batch, then lx_abft_restore."""
        creator = np.ascontiguousarray(creator, dtype=np.uint32)
        seq = np.ascontiguousarray(seq, dtype=np.uint32)
        poff = np.ascontiguousarray(poff, dtype=np.uint64)
        par = np.ascontiguousarray(par if len(par) else [0], dtype=np.uint32)
        n = len(creator)
        self.ix.reset(self.weights)
        for lo in range(0, n, chunk):
            hi = min(n, lo + chunk)
            self.ix.load_rows(creator[lo:hi], seq[lo:hi], poff[lo:hi + 1] - poff[lo], par[int(poff[lo]):int(poff[hi])],
                              b"".join(tables["b"][k] for k in range(lo, hi)),
                              [tables["S"][k] for k in range(lo, hi)], [tables["s"][k] for k in range(lo, hi)])
        if n or tables.get("B"):
            self.ix.load_finish(tables.get("B", b""))
        self._chk(restore_arrays(self.L, self.h, state, self.weights, creator, seq, poff, par, self._cb))

    def close(self):
        if getattr(self, "h", None):
            self.L.lx_abft_destroy(self.h)
            self.h = None
        if getattr(self, "ix", None) is not None:
            self.ix.close()

    __del__ = close

    def _begin(self, user, frame, atropos, cheaters, n):
        self._cur = [self.epoch(), frame, atropos, tuple(cheaters[k] for k in range(n)), []]

    def _apply(self, user, ev):
        self._cur[4].append(ev)

    def _end(self, user, n_out, w_out):
        b = self._cur
        self.blocks.append((b[0], b[1], b[2], b[3], tuple(b[4])))
        nw = self.seal(b[0], b[1]) if self.seal else None
        if nw is None:
            return 0
        self._seal_w = np.ascontiguousarray(nw, dtype=np.uint32)
        n_out[0] = len(self._seal_w)
        w_out[0] = self._seal_w.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
        return 1

    def process_batch(self, creator, seq, poff, par, claimed=None):
        """Returns (rc, consumed, frames)."""
        creator = np.ascontiguousarray(creator, dtype=np.uint32)
        seq = np.ascontiguousarray(seq, dtype=np.uint32)
        poff = np.ascontiguousarray(poff, dtype=np.uint64)
        par = np.ascontiguousarray(par if len(par) else [0], dtype=np.uint32)
        n = len(creator)
        out = np.zeros(n, dtype=np.uint32)
        cl = None if claimed is None else np.ascontiguousarray(claimed, dtype=np.uint32)
        consumed = ctypes.c_uint32()
        rc = self.L.lx_abft_process_batch(self.h, n, _p(creator, u32p), _p(seq, u32p), _p(poff, u64p),
                                          _p(par, u32p), None if cl is None else _p(cl, u32p), _p(out, u32p),
                                          ctypes.byref(consumed))
        if rc not in (0, ERR_FRAME):
            raise LxError(rc, self.L.lx_abft_last_error(self.h).decode())
        if self.block_log:
            self._read_block_log()
        return rc, consumed.value, out

    def _read_block_log(self):
        nb = ctypes.c_uint32()
        ptr = [ctypes.POINTER(ctypes.c_uint32)() for _ in range(6)]
        rc = self.L.lx_abft_block_log(self.h, ctypes.byref(nb), *[ctypes.byref(q) for q in ptr])
        if rc != 0:
            raise LxError(rc, self.L.lx_abft_last_error(self.h).decode())
        n = nb.value
        if not n:
            return
        fr, at, co, ch, fo, cf = ptr
        ep = self.epoch()
        for k in range(n):
            self.blocks.append((ep, fr[k], at[k], tuple(ch[i] for i in range(co[k], co[k + 1])),
                                tuple(cf[i] for i in range(fo[k], fo[k + 1]))))

    def build(self, creator, seq, parents):
        """lx_abft_build: the frame of one event (added, evaluated, dropped)."""
        p = np.ascontiguousarray(parents if len(parents) else [0], dtype=np.uint32)
        out = ctypes.c_uint32()
        self._chk(self.L.lx_abft_build(self.h, int(creator), int(seq), len(parents), _p(p, u32p), ctypes.byref(out)))
        return out.value

    def build_frames(self, creator, seq, poff, par):
        """lx_abft_build_frames: (rc, err_index, frames, is_root) of candidate
        events that are not added."""
        return build_frames_arrays(self.L, self.h, creator, seq, poff, par)

    def build_progress(self, creator, seq, poff, par, at_frame=None, pairs=False, flags=None):
        """lx_abft_build_progress: (rc, err_index, dict of arrays ``frame``,
        ``n_roots``, ``n_caused``, ``stake``, ``root_stake``) of candidate
        events that are not added."""
        return build_progress_arrays(self.L, self.h, creator, seq, poff, par, at_frame, pairs, flags=flags)

    def event_progress(self, events, at_frame=None, pairs=False, flags=None):
        """lx_abft_event_progress: the same for indexed events."""
        return event_progress_arrays(self.L, self.h, events, at_frame, pairs, flags=flags)

    def progress_pairs(self, n, cap=None):
        """lx_abft_last_progress_pairs after a progress call of n entries:
        (pair_off, root events, stakes, n_pairs)."""
        return progress_pairs(self.L, self.h, n, cap)

    def build_stats(self):
        """lx_abft_build_last_stats."""
        st = BuildStats()
        self._chk(self.L.lx_abft_build_last_stats(self.h, ctypes.byref(st)))
        return {f: getattr(st, f) for f, _ in BuildStats._fields_}

    def epoch(self):
        return self.L.lx_abft_epoch(self.h)

    def confirmed_on(self, n):
        """GetEventConfirmedOn of events [0, n) of the epoch (0 = not confirmed)."""
        out = np.zeros(n, dtype=np.uint32)
        f = ctypes.c_uint32()
        for i in range(n):
            rc = self.L.lx_abft_event_confirmed_on(self.h, i, ctypes.byref(f))
            if rc != 0:
                raise LxError(rc, self.L.lx_abft_last_error(self.h).decode())
            out[i] = f.value
        return out

    def last_decided_frame(self):
        return self.L.lx_abft_last_decided_frame(self.h)

    def frame_roots(self, f):
        n = ctypes.c_uint32()
        self.L.lx_abft_frame_roots(self.h, f, None, 0, ctypes.byref(n))
        out = np.zeros(max(n.value, 1), dtype=np.uint32)
        self.L.lx_abft_frame_roots(self.h, f, _p(out, u32p), n.value, ctypes.byref(n))
        return out[:n.value]

    def last_stats(self):
        st = AbftStats()
        self.L.lx_abft_last_stats(self.h, ctypes.byref(st))
        return {f: getattr(st, f) for f, _ in AbftStats._fields_}

    def set_option(self, name, value):
        """lx_abft_set_option (path selection; results never change)."""
        rc = self.L.lx_abft_set_option(self.h, name.encode(), int(value))
        if rc != 0:
            raise LxError(rc, self.L.lx_abft_last_error(self.h).decode())
