"""The scenarios of tests/claim_dags.py are what tests/test_gpu_abft_claims.py
needs -- asserted from the oracle alone (Process per event), so that a change
of a generator cannot silently empty the GPU test.  CPU only.

The conditions are thresholds, not the measured counts.  Measured with the
generators as they are: lowballed epochs lower 19 - 148 claims, give 4 - 36
blocks against 6 - 38 honest ones and move the frame of at least 239 of 600
events (shape A, every 3rd root less one: 27 lowered, 17 / 22 blocks, 111 of
120 frames); mutated cases, as rejected at a mutated event / between mutated
events / behind all of them at an honest event / accepted whole: A 30 / 2 / 3 /
1, B 31 / 2 / 1 / 2, C 31 / 1 / 0 / 4, D 34 / 0 / 1 / 1; the ladder asks for
2,102 frame steps at V = 64 and 33,145 at V = 256 and is refused at its first
event; the sealed tail seals at event 85 of 600.
"""

from collections import Counter

import pytest

import claim_dags as cd


@pytest.mark.parametrize("every,drop", cd.LOW_MODES)
@pytest.mark.parametrize("shape", sorted(cd.SHAPES))
def test_lowballed_epochs_are_accepted_and_differ(shape, every, drop):
    hon = cd.honest(shape)
    r = cd.lowballed(shape, every, drop)
    assert r["err"] is None and len(r["claims"]) == r["n"]
    assert len(r["blocks"]) >= 3
    assert r["lowered"] >= 15
    moved = sum(1 for k, f in r["frames"].items() if f != hon["frames"][k])
    assert 4 * moved >= r["n"]
    assert r["blocks"] != hon["blocks"]


def test_mutated_cases_cover_every_outcome():
    total = Counter()
    rejected, accepted = Counter(), Counter()
    for shape in sorted(cd.SHAPES):
        per = Counter()
        for case in range(cd.N_CASES):
            m = cd.mutated(shape, case)
            assert 1 <= len(m["muts"]) <= 3
            hon = cd.honest(shape)["frames"]
            assert sum(1 for k in hon if m["claims"][k] != hon[k]) == len(m["muts"])
            per[m["outcome"]] += 1
            for i, kind in m["muts"].items():
                if m["consumed"] == i:
                    rejected[kind] += 1
                elif m["consumed"] > i:
                    accepted[kind] += 1
        assert per["at_mutated"] >= 20, (shape, per)
        total += per
    assert total["later"] >= 4, total      # at an honest event behind every mutated one
    assert total["accepted"] >= 3, total
    assert all(rejected[k] >= 1 for k in cd.KINDS), rejected
    assert accepted["-1"] >= 1 and accepted["spf"] >= 1, accepted


def test_mutated_first_events():
    """Every sixth case mutates a creator's first event."""
    from oracle import abft_oracle as ao
    for shape in sorted(cd.SHAPES):
        _, evs = cd.shape_events(shape)
        for case in range(5, cd.N_CASES, 6):
            m = cd.mutated(shape, case)
            assert any(ao.self_parent(evs[i]) is None for i in m["muts"])


def test_ladder_is_refused_early_and_grows_quadratically():
    small, big = cd.ladder(64), cd.ladder(256)
    for l in (small, big):
        assert l["consumed"] < 2
        assert l["n"] == 4 * l["V"]
    assert big["steps"] > 8 * small["steps"]


def test_mass_return_exceeds_one_pass():
    """Honest claims: the return level alone asks for more frame steps than
    one pass takes (450 against 304), the whole epoch for fewer (640 against
    2,184) -- an honest epoch in one batch is not cut."""
    import election_dags as ed
    w, d, lo, hi = cd.mass_return()
    ref = ed.oracle_run(w, d)
    assert hi - lo == len(w) and len(ref["blocks"]) >= 3
    assert cd.claimed_steps(d, ref["frames"], lo, hi) > cd.pass_budget(hi - lo, len(w))
    assert cd.claimed_steps(d, ref["frames"], 0, len(d)) <= cd.pass_budget(len(d), len(w))


@pytest.mark.parametrize("kind", cd.TAIL_KINDS)
def test_sealed_tail_seals_inside_the_batch(kind):
    r = cd.sealed_tail(kind)
    assert 0 < r["consumed"] and r["n"] - r["consumed"] >= 100
    assert r["last"] == (2, 0) and len(r["blocks"]) == cd.TAIL_SEAL_FRAME
    assert r["consumed"] <= cd.TAIL_BAD < r["n"]
    _, evs = cd.tail_events()
    tail = [r["claims"][e.id] for e in evs[r["consumed"]:]]
    head = [r["claims"][e.id] for e in evs[:r["consumed"]]]
    assert head == [cd.sealed_tail("honest")["claims"][e.id] for e in evs[:r["consumed"]]]
    if kind == "one":
        assert set(tail) == {1}
    elif kind == "build":
        assert set(tail) == {cd.FRAME_BUILD}
    elif kind == "top2":
        hon = cd.sealed_tail("honest")["claims"]
        assert [e.id for e in evs if r["claims"][e.id] != hon[e.id]] == [evs[cd.TAIL_BAD].id]
    assert len(r["epoch2"]["blocks"]) > len(r["blocks"])
