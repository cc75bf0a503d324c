"""The abft engine against the C oracle on the scheduled-participation DAGs of
tests/election_dags.py: elections whose first subject window [0, 64) is decided
"no" throughout (widen_window, vote_slots with v_lo > 0, the hand-over of the
elections decided ahead), elections of up to 9 rounds (past the 8 rounds
elect_ahead may take), returning validators whose first event holds root
slots of several frames, and an election whose first decider within the rounds
voted ahead is younger than its true one (lagger_return, seen through a seal).  tests/test_election_dags.py asserts from the oracle
alone that the scenarios reach these branches.

Compared: the frame of every event, the roots of every frame (as sets: a
frame's slots are listed in the order they were found, and a batch finds the
slots a returning validator's event holds in the frames it passes at another
step than event-by-event processing does; the reference lists them in its
store's key order, and without forks no result depends on the order), every
block (frame, Atropos, cheaters, confirmed events in ApplyEvent order) and the
last decided frame -- for elect_ahead 0 / 2 / 3 / 8, frames computed or claimed
(claimed_batch 1 and 0), the epoch in one batch, in 7 chunks and (head_silent_
return) cut at every level boundary from the start of the outage on: the cut
that leaves an older slot unvoted when a decision is read.

Measured on an MI355X, per parametrised case with all modes and cuts of it:
the first case of a scenario, which also generates the DAG and computes the
oracle's answer once, 2.5 s (head_silent_return), 1.3 s (head_never_two),
0.25 s (head_never), 0.15 s or less (long_rounds*); every later case of a
scenario 0.03 - 0.13 s; an event-by-event case 0.03 - 0.05 s; a seal case
under 0.01 s.  The module: 55 tests in 6.3 s.
"""

import numpy as np
import pytest

import election_dags as ed
from abft_harness import FakeLachesis

pytestmark = pytest.mark.gpu

_cache = {}


def reference(name):
    if name not in _cache:
        w, d = ed.scenario(name)
        _cache[name] = (w, d, ed.oracle_run(w, d))
    return _cache[name]


def cuts_of(name, d):
    n = len(d)
    out = {"whole": [0, n], "chunks7": np.linspace(0, n, 8).astype(np.int64).tolist()}
    if name == "head_silent_return":
        out["levels"] = [0] + [int(x) for x in d.level_ends[ed.OUTAGE[0]:]]
    return out


def run_gpu(w, d, bounds, claim, options):
    """(frames, roots per frame, blocks, last decided frame, elections decided ahead)."""
    from lachesis_hip import abft
    lch = abft.DenseLachesis(w, event_capacity=len(d))
    try:
        for k, v in options.items():
            lch.set_option(k, v)
        frames = np.zeros(len(d), dtype=np.uint32)
        ahead = 0
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            rc, consumed, out = lch.process_batch(*d.slice(lo, hi), claimed=None if claim is None else claim[lo:hi])
            assert rc == 0 and consumed == hi - lo
            frames[lo:hi] = out
            ahead += lch.last_stats()["elections_ahead"]
        nf = int(frames.max()) + 1
        return frames, [sorted(lch.frame_roots(f).tolist()) for f in range(nf + 1)], list(lch.blocks), \
            lch.last_decided_frame(), ahead
    finally:
        lch.close()


@pytest.mark.parametrize("elect_ahead", [0, 2, 3, 8])
@pytest.mark.parametrize("name", ed.SCENARIOS)
def test_engine_matches_oracle(name, elect_ahead):
    w, d, ref = reference(name)
    assert len(ref["blocks"]) >= 2
    for cut, bounds in cuts_of(name, d).items():
        for mode, claim, cb in (("computed", None, 1), ("claimed", ref["frames"], 1), ("claimed0", ref["frames"], 0)):
            tag = (cut, mode)
            frames, roots, blocks, last, ahead = run_gpu(w, d, bounds, claim,
                                                         {"elect_ahead": elect_ahead, "claimed_batch": cb})
            assert np.array_equal(frames, ref["frames"]), tag
            assert roots == [sorted(r) for r in ref["roots"]], tag
            assert blocks == ref["blocks"], tag
            assert last == ref["last"], tag
            if elect_ahead == 0:
                assert ahead == 0, tag
            elif name.startswith("head_never"):
                # every election's Atropos lies past the first window: the
                # ahead path must hand each of them over
                assert ahead == 0, tag
            elif name == "long_rounds" and elect_ahead == 8 and cut == "whole":
                assert ahead > 0, tag


@pytest.mark.parametrize("elect_ahead", [0, 2, 8])
@pytest.mark.parametrize("name", [n for n in ed.SCENARIOS if n.startswith("long_rounds")])
def test_long_rounds_event_by_event(name, elect_ahead):
    """One lx_abft_process_batch call per event through the harness of the
    reference's own tests: the block appears at the same event."""
    w, d, _ = reference(name)
    wmap, evs = ed.as_events(w, d)
    ref = FakeLachesis(wmap)
    got = FakeLachesis(wmap, backend="gpu", options={"elect_ahead": elect_ahead})
    for e in evs:
        ref.build(e)
        assert ref.process(e) is None
        want_frame, e.frame = e.frame, 0
        consumed, err = got.process_batch([e], claimed=False)
        assert err is None and consumed == 1
        assert e.frame == want_frame, e
        assert got.block_list == ref.block_list, e
    assert got.store.last_decided_frame == ref.store.last_decided_frame
    assert len(ref.block_list) >= 13


@pytest.mark.parametrize("elect_ahead", [0, 2, 3, 8])
def test_seal_at_the_older_decider(elect_ahead):
    """lagger_return, the epoch sealed by block 3, whole epoch in one batch:
    within two rounds election 3 is first decided by event 48, but event 45 (a
    root of frame 6, round 3) decides it earlier -- a decision read from the
    rounds voted ahead is final only if no slot left unvoted is older.  The
    seal shows the deciding event: the batch is consumed up to it."""
    from lachesis_hip import abft
    w, d = ed.scenario("lagger_return")
    seal = lambda epoch, frame: w if frame == 3 else None
    ref = ed.oracle_run(w, d, seal=seal)
    assert ref["consumed"] == 46
    lch = abft.DenseLachesis(w, event_capacity=len(d), seal=seal)
    try:
        lch.set_option("elect_ahead", elect_ahead)
        rc, consumed, out = lch.process_batch(*d.slice(0, len(d)))
        assert rc == 0 and consumed == ref["consumed"]
        assert np.array_equal(out[:consumed], ref["frames"])
        assert lch.blocks == ref["blocks"] and lch.epoch() == ref["epoch"] == 2
    finally:
        lch.close()
