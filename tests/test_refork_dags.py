"""The re-fork scenarios of tests/refork_dags.py discriminate: pinned to the
oracle (vecfc_oracle.Index with add / flush / drop_not_flushed,
abft_harness.FakeLachesis, emitter_oracle.QuorumIndexer) on the CPU, so that
tests/test_gpu_refork.py compares the library on inputs where a table kept
from before the rollback gives another answer.  A scenario that misses a
condition is regenerated with the next seed (refork_dags.found), never
skipped; the conditions are asserted here on what it returned."""

import pytest

import refork_dags as rd
from oracle import emitter_oracle as eo

NAMES = list(rd.VARIANTS)


@pytest.mark.parametrize("name", NAMES)
def test_variant_shape(name):
    V, X, Y, n, with_z, two = rd.VARIANTS[name]
    sc = rd.get(name)
    assert (sc.V, sc.X, sc.Y) == (V, X, Y) and X != Y
    assert len(sc.A) == len(sc.A2) == n
    assert len(sc.P) + len(sc.A2) + len(sc.T) < 100          # tens of events
    o, bx = rd.drive_oracle(sc)
    bi = o.branches_info()
    # X forks in A and stays honest afterwards; Y (and W) fork in A2
    assert len(bi.by_creators[X]) == 1 and len(bi.by_creators[Y]) == 2
    first = V + (1 if with_z else 0)
    assert bx == list(range(first, first + (2 if two else 1)))
    assert (sc.Z is not None) == with_z and (not with_z or len(bi.by_creators[sc.Z]) == 2)
    if two:
        assert len(bi.by_creators[sc.W]) == 2 and sc.W not in (X, Y)
        assert [bi.creator_idxs[b] for b in bx] == [Y, sc.W]
    assert all(e.creator - 1 != X or e.id not in sc.fork_branch_ids for e in sc.A2 + sc.T)


def test_variants_cover_the_issue():
    v = rd.VARIANTS.values()
    assert {x[0] for x in v} == {4, 5, 8}
    assert any(x[2] < x[1] for x in v) and any(x[2] > x[1] for x in v)
    assert any(x[3] == 1 for x in v) and any(24 <= x[3] <= 48 for x in v)
    assert any(x[4] for x in v) and any(x[5] for x in v)
    split = rd.shard_split(8)
    assert split == 4
    sides = {(x[1] < split, x[2] < split) for x in v if x[0] == 8}
    assert (True, False) in sides and (False, True) in sides
    assert any(x[0] == 8 and x[3] == 1 and (x[1] < split) != (x[2] < split) for x in v)


@pytest.mark.parametrize("name", NAMES)
def test_same_branch_number_other_creator(name):
    sc = rd.get(name)
    o, bx = rd.drive_oracle(sc)
    assert [o.get_event_branch_id(f.id) for f in sc.fy] == bx
    assert all(o.branches_info().creator_idxs[b] != sc.X for b in bx)


@pytest.mark.parametrize("name", NAMES)
def test_merged_rows_need_the_new_map(name):
    sc = rd.get(name)
    o, _ = rd.drive_oracle(sc)
    X, Y = sc.X, sc.Y
    fork_col = o.get_event_branch_id(sc.fy[0].id)
    # (a): one parent on Y's fork branch; merged HB[Y] comes from the fork column
    assert sum(1 for p in sc.ea.parents if p in sc.fork_branch_ids) == 1
    hb, m = o.get_highest_before(sc.ea.id), o.get_merged_highest_before(sc.ea.id)
    assert m.get(Y)[0] == hb.get(fork_col)[0] > hb.get(Y)[0]
    # (b): both branches of Y, none of X's doing
    m = o.get_merged_highest_before(sc.eb.id)
    assert m.is_fork_detected(Y) and not m.is_fork_detected(X)
    # (c): an event of X under both
    assert sc.xc.creator - 1 == X
    for e in (sc.ea, sc.eb):
        assert o.get_highest_before(e.id).get(X)[0] >= sc.xc.seq
    # the emitter's matrix: the column of (a)'s creator holds Y's fork-branch seq
    q = eo.QuorumIndexer(sc.validators, o, eo.capped_metric(sc.validators.weights, 2))
    q.process_event(sc.ea, True)
    assert q.get_global_matrix()[Y][sc.me] == hb.get(fork_col)[0]


@pytest.mark.parametrize("name", NAMES)
def test_forkless_cause_on_the_quorum_edge(name):
    sc = rd.get(name)
    o, bx = rd.drive_oracle(sc)
    o0, _ = rd.drive_oracle(sc, "nofork")
    a, b = sc.ea2.id, sc.xc.id
    assert o.forkless_cause(a, b) is True
    assert o0.forkless_cause(a, b) is False                    # Y's stake, through the fork column, decides
    assert rd.stale_forkless_cause(o, sc, a, b, bx) is False   # credited to X it is lost
    assert rd.stale_forkless_cause(o, sc, a, b, []) is True
    kept = [e.id for e in sc.without_fork()]
    diff = sum(o.forkless_cause(x, y) != o0.forkless_cause(x, y) for x in kept for y in kept)
    assert diff >= 1


@pytest.mark.parametrize("name", NAMES)
def test_abft_frames_depend_on_the_fork(name):
    sc = rd.get(name, abft=True)
    assert rd.discriminates(sc, abft=True) is None
    f1, f0 = rd.frames_of(sc, sc.A2 + sc.T), rd.frames_of(sc, sc.without_fork())
    assert any(f1[k] != f0[k] for k in f0)


def test_reshuffled_redo_changes_owners():
    validators, store, ops = rd.reshuffled()
    assert rd.owner_changes(validators, store, ops) >= 3
    drops = sum(1 for op in ops if op[0] == "drop")
    assert drops >= 3 and ops[-1] == ("flush",)
    # every event is added (and kept) exactly once in the end
    kept, pending = [], []
    for op in ops:
        if op[0] == "add":
            pending += op[1]
        elif op[0] == "flush":
            kept += pending
            pending = []
        else:
            pending = []
    assert sorted(e.id for e in kept) == sorted(store)
