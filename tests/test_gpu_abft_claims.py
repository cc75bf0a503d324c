"""lx_abft_process_batch on claimed frames that are low, wrong, inflated or lie
behind a seal (tests/claim_dags.py; tests/test_claim_dags.py asserts from the
oracle alone that the scenarios are what this module needs).  The claims are
untrusted input; the oracle is Process per event on the same claims
(abft_harness.FakeLachesis), computed once per scenario.

* Lowballed epochs: roots that claim less than their true frame are accepted
  (calcFrameIdx takes the claim as its loop bound) and the epoch goes on with
  other roots, frames and blocks -- the batched path derives its root lists,
  bit-row positions and bm_len from exactly these claims.  Every event's frame,
  every block and (epoch, last decided frame) equal the oracle's.
* Mutated cases: one to three wrong claims of nine kinds.  The position of the
  first rejection (at the mutated event, at a later honest one, or none), the
  frames and blocks up to it, and the epoch continued from the rejected event
  with Build semantics -- the index and the engine after restore_snapshot +
  lx_drop_not_flushed, forks present.
* Sealed tail: a seal inside the batch with 514 events behind it that claim
  next-epoch-like, constant, inflated or LX_FRAME_BUILD frames; then an honest
  epoch-2 DAG.
* Ladder: V events claiming top + 1 + k.  Result parity, and the work: R(V) =
  fc_pairs of the ladder call / fc_pairs of the honest call for the same V
  events on a handle in the same state; R(256) <= 2 R(64).  A path that queues
  every claimed step before it verifies one has R grow like V.
* Mass return: an honest batch whose climbs exceed one pass's step budget is
  processed in several passes inside the call, with the oracle's results.

Ladder work, fc_pairs of the ladder call / of the honest call (both read from
last_stats(), cleared per call, discarded speculative work included):

                         V = 64            V = 256          R(64)   R(256)
    passes of 2n+4V+64   10,232 / 1,408    72,930 / 55,552   7.27    1.31
    every step queued    92,864 / 1,408    5,721,600 / 55,552  65.95  103.00

The second row is the library before the budget (all 2,102 and 33,145 frame
steps of claim_dags.ladder queued at once).  Its R grows 1.56x, not the ~3x a
host-side estimate gave: honest pairs grow 39x from V = 64 to 256 because the
rounds are four events deep, so R(256) <= 2 R(64) holds on both rows and only
the budget bound of test_ladder_work_is_bounded tells them apart (28,672 +
1,408 and 409,600 + 55,552 pairs allowed).

The sealed tail found a bug: with a wrong claim on the first event behind the
seal (kind "one": event 86 claims 1) the redo of the events before it ends
exactly at the sealing event, and the call reported LX_ERR_FRAME for an event
of the next epoch instead of the seal.

Measured on an MI355X: the module, 177 tests, 11.3 s; the first lowballed case
(which starts the device) 1.7 s, test_ladder_round_matches_oracle[256] 0.5 s,
every other case 0.25 s or less.
"""

import numpy as np
import pytest

import claim_dags as cd
from abft_harness import FakeLachesis

pytestmark = pytest.mark.gpu


def gpu(wmap, options=None):
    return FakeLachesis(wmap, backend="gpu", options=options or {})


def feed(t, evs, claims=None, chunk=None):
    """Batches of ``chunk`` events (None: one batch) on the given claims
    ({event id: frame}; None = Build semantics) until the first error or seal:
    (events consumed, error)."""
    epoch = t.store.get_epoch()
    i = 0
    while i < len(evs):
        part = evs[i:i + (chunk or len(evs))]
        if claims is not None:
            for e in part:
                e.frame = claims[e.id]
        consumed, err = t.process_batch(part, claimed=claims is not None)
        i += consumed
        if err is not None or t.store.get_epoch() != epoch:
            return i, err
        assert consumed == len(part)
    return i, None


def state(t):
    return dict(blocks=list(t.block_list), last=(t.store.get_epoch(), t.store.last_decided_frame))


def frames_of(t, evs):
    return {e.id: t.lch.frame_of(e.id) for e in evs}


LOW_COMBOS = [
    # claimed_batch, chunk, elect_ahead, fc16 (None: default)
    (1, None, 3, None), (1, 7, 3, None), (1, 64, 0, None), (0, None, 0, None), (1, None, 3, 0),
]


@pytest.mark.parametrize("every,drop", cd.LOW_MODES)
@pytest.mark.parametrize("shape", sorted(cd.SHAPES))
def test_lowballed_epoch_matches_oracle(shape, every, drop):
    ref = cd.lowballed(shape, every, drop)
    assert ref["err"] is None
    for cb, chunk, ea, fc16 in LOW_COMBOS:
        opts = {"claimed_batch": cb, "elect_ahead": ea}
        if fc16 is not None:
            opts["fc16"] = fc16
        wmap, evs = cd.shape_events(shape)
        t = gpu(wmap, opts)
        try:
            consumed, err = feed(t, evs, ref["claims"], chunk)
            assert err is None and consumed == ref["n"], (cb, chunk, ea, fc16)
            assert frames_of(t, evs) == ref["frames"], (cb, chunk, ea, fc16)
            got = state(t)
            assert got["blocks"] == ref["blocks"], (cb, chunk, ea, fc16)
            assert got["last"] == ref["last"], (cb, chunk, ea, fc16)
        finally:
            t.lch.close()


@pytest.mark.parametrize("case", range(cd.N_CASES))
@pytest.mark.parametrize("shape", sorted(cd.SHAPES))
def test_mutated_claims_first_error_and_continuation(shape, case):
    ref = cd.mutated(shape, case)
    for cb in (1, 0):
        for chunk in (None, 7):
            wmap, evs = cd.shape_events(shape)
            t = gpu(wmap, {"claimed_batch": cb})
            try:
                consumed, err = feed(t, evs, ref["claims"], chunk)
                assert consumed == ref["consumed"], (cb, chunk, ref["muts"])
                assert (err is None) == (consumed == ref["n"]), (cb, chunk)
                assert frames_of(t, evs[:consumed]) == ref["frames"], (cb, chunk)
                got = state(t)
                assert got["blocks"] == ref["blocks"] and got["last"] == ref["last"], (cb, chunk)
                # the epoch goes on from the rejected event, frames computed
                rest, err = feed(t, evs[consumed:], None, chunk and 64)
                assert err is None and rest == ref["n"] - consumed, (cb, chunk)
                got = state(t)
                assert got["blocks"] == ref["final"]["blocks"], (cb, chunk)
                assert got["last"] == ref["final"]["last"], (cb, chunk)
            finally:
                t.lch.close()


@pytest.mark.parametrize("claimed_batch", [1, 0])
@pytest.mark.parametrize("cut", [None, 64])
@pytest.mark.parametrize("kind", cd.TAIL_KINDS)
def test_sealed_tail(kind, cut, claimed_batch):
    ref = cd.sealed_tail(kind)
    wmap, evs = cd.tail_events()
    t = gpu(wmap, {"claimed_batch": claimed_batch})
    try:
        cd.seal_at(t, cd.TAIL_SEAL_FRAME)
        consumed = 0
        if cut:
            consumed, err = feed(t, evs[:cut], ref["claims"])
            assert err is None and consumed == cut < ref["consumed"]
        c, err = feed(t, evs[consumed:], ref["claims"])
        assert err is None
        assert consumed + c == ref["consumed"]
        got = state(t)
        assert got["blocks"] == ref["blocks"] and got["last"] == ref["last"]
        t.apply_block = None
        e2 = cd.tail_epoch2()
        c2, err = feed(t, e2)
        assert err is None and c2 == len(e2)
        assert {e.id: e.frame for e in e2} == ref["epoch2"]["frames"]
        got = state(t)
        assert got["blocks"] == ref["epoch2"]["blocks"] and got["last"] == ref["epoch2"]["last"]
    finally:
        t.lch.close()


_ladder_runs = {}


def ladder_run(V):
    """The ladder round after its honest prefix (an earlier call): parity with
    the oracle, then the round again on honest claims; fc_pairs of the ladder
    call and of the honest call on a second handle in the same state."""
    if V in _ladder_runs:
        return _ladder_runs[V]
    ref = cd.ladder(V)
    out = {}
    for which in ("ladder", "honest"):
        wmap, evs = cd.ladder_events(V)
        prefix, rnd = evs[:-V], evs[-V:]
        t = gpu(wmap)
        try:
            consumed, err = feed(t, prefix, ref["honest"])
            assert err is None and consumed == len(prefix)
            if which == "ladder":
                consumed, err = feed(t, rnd, ref["claims"])
                out["ladder_pairs"] = t.lch.last_stats()["fc_pairs"]
                out["ladder_steps"] = t.lch.last_stats()["frame_steps"]
                assert consumed == ref["consumed"] and err is not None
                assert frames_of(t, rnd[:consumed]) == ref["frames"]
                got = state(t)
                assert got["blocks"] == ref["blocks"] and got["last"] == ref["last"]
                rnd = rnd[consumed:]
            consumed, err = feed(t, rnd, ref["honest"])
            if which == "honest":
                out["honest_pairs"] = t.lch.last_stats()["fc_pairs"]
                out["honest_steps"] = t.lch.last_stats()["frame_steps"]
            assert err is None and consumed == len(rnd)
            assert frames_of(t, evs) == ref["honest"]
            got = state(t)
            assert got["blocks"] == ref["full"]["blocks"] and got["last"] == ref["full"]["last"]
        finally:
            t.lch.close()
    _ladder_runs[V] = out
    return out


@pytest.mark.parametrize("V", [64, 256])
def test_ladder_round_matches_oracle(V):
    r = ladder_run(V)
    print("ladder V=%d fc_pairs ladder %d honest %d, frame_steps ladder %d honest %d" %
          (V, r["ladder_pairs"], r["honest_pairs"], r["ladder_steps"], r["honest_steps"]))
    assert r["ladder_pairs"] > 0 and r["honest_pairs"] > 0


def test_ladder_whole_epoch_in_one_call():
    V = 64
    ref = cd.ladder(V)
    wmap, evs = cd.ladder_events(V)
    t = gpu(wmap)
    try:
        consumed, err = feed(t, evs, ref["claims"])
        assert consumed == len(evs) - V + ref["consumed"] and err is not None
        assert frames_of(t, evs[:consumed]) == {e.id: ref["claims"][e.id] for e in evs[:consumed]}
        got = state(t)
        assert got["blocks"] == ref["blocks"] and got["last"] == ref["last"]
        rest, err = feed(t, evs[consumed:], ref["honest"])
        assert err is None and rest == len(evs) - consumed
        got = state(t)
        assert got["blocks"] == ref["full"]["blocks"] and got["last"] == ref["full"]["last"]
    finally:
        t.lch.close()


def test_ladder_work_is_bounded():
    """R(V) = fc_pairs(ladder call) / fc_pairs(honest call).  Honest work per
    event grows with V on both sides of the ratio, so a bounded path keeps R
    about constant; queueing every claimed step makes it grow like V (about 3x
    from 64 to 256).  The factor 2 sits between the two."""
    r64, r256 = ladder_run(64), ladder_run(256)
    R64 = r64["ladder_pairs"] / r64["honest_pairs"]
    R256 = r256["ladder_pairs"] / r256["honest_pairs"]
    print("R(64) = %.3f, R(256) = %.3f" % (R64, R256))
    assert R256 <= 2 * R64
    # The ratio alone does not tell the two paths apart (module docstring:
    # honest pairs grow 39x from 64 to 256, so the unbounded path passes it
    # too).  The documented budget does: one pass queues at most
    # pass_budget(n, V) frame steps, a step pairs one candidate with at most
    # one root slot per validator (no forks here), and what the refused call
    # processes besides (the verified events before the refused one, at most
    # one here) is honest work.
    for V, r in ((64, r64), (256, r256)):
        assert r["ladder_pairs"] <= cd.pass_budget(V, V) * V + r["honest_pairs"], V


def test_mass_return_is_processed_in_passes():
    """An honest batch over the step budget of one pass (30 validators back
    from a long outage in one level): cut for budget, never refused, the
    oracle's frames, roots and blocks -- and more than one root-FC launch in
    the call, one per pass."""
    from lachesis_hip import abft
    import election_dags as ed
    w, d, lo, hi = cd.mass_return()
    ref = ed.oracle_run(w, d)
    steps = cd.claimed_steps(d, ref["frames"], lo, hi)
    assert steps > cd.pass_budget(hi - lo, len(w))
    lch = abft.DenseLachesis(w, event_capacity=len(d))
    try:
        frames = np.zeros(len(d), dtype=np.uint32)
        for a, b in ((0, lo), (lo, hi), (hi, len(d))):
            rc, consumed, out = lch.process_batch(*d.slice(a, b), claimed=ref["frames"][a:b])
            assert rc == 0 and consumed == b - a
            frames[a:b] = out
            if a == lo:
                st = lch.last_stats()
                assert st["fc_launches"] >= 2
        assert np.array_equal(frames, ref["frames"])
        nf = int(frames.max()) + 1
        assert [sorted(lch.frame_roots(f).tolist()) for f in range(nf + 1)] == [sorted(r) for r in ref["roots"]]
        assert list(lch.blocks) == ref["blocks"] and lch.last_decided_frame() == ref["last"]
    finally:
        lch.close()
