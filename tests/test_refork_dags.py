"""The re-fork scenarios of tests/refork_dags.py discriminate: pinned to the
oracle (vecfc_oracle.Index with add / flush / drop_not_flushed,
abft_harness.FakeLachesis, emitter_oracle.QuorumIndexer) on the CPU, so that
tests/test_gpu_refork.py compares the library on inputs where a table kept
from before the rollback gives another answer.  A scenario that misses a
condition is regenerated with the next seed (refork_dags.found), never
skipped; the conditions are asserted here on what it returned.

The readers that tests/test_gpu_refork_readers.py drives (MedianTime,
ancestry, fork evidence, Build / frame progress) have one condition each:
some query's right answer differs from the answer computed with the fork
columns of ``A`` still credited to X.  All nine variants meet all four."""

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


# ---------------------------------------------------------------------------- per reader

@pytest.mark.parametrize("name", NAMES)
def test_median_time_needs_the_new_map(name):
    """Creation times chosen so that MedianTime(ea) and MedianTime(eb) both
    differ, under either default, with the fork column credited to X: at ea the
    entry of Y comes from the fork column, at eb Y is a cheater and X is not."""
    sc = rd.get(name)
    t = rd.times_of(name)
    assert t is not None, "no creation times discriminate for MedianTime in %s" % name
    assert set(t) == set(sc.store)
    diffs = rd.median_time_diffs(sc, t)
    assert {(h, d) for h, d, _, _ in diffs} == {(h.id, d) for h in (sc.ea, sc.eb) for d in rd.MT_DEFAULTS}
    # the dropped events' times are others than those of the events re-added at their indices
    assert any(t[a.id] != t[b.id] for a, b in zip(sc.A, sc.A2))
    o, bx = rd.drive_carried(sc, t)
    _, stale_by = rd.stale_map(o, sc, bx)
    import median_time_model as mm
    Y = sc.Y
    right, stale = o.merged(sc.ea.id), rd.merged_times_by_map(o, sc.ea.id, stale_by)
    assert right[Y] == (mm.SEEN, t[sc.fy[0].id]) and stale[Y] != right[Y]
    right, stale = o.merged(sc.eb.id), rd.merged_times_by_map(o, sc.eb.id, stale_by)
    assert right[Y][0] == mm.FORK and right[sc.X][0] == mm.SEEN and stale[sc.X][0] == mm.FORK


@pytest.mark.parametrize("name", NAMES)
def test_ancestry_needs_the_new_map(name):
    """observes(eb, fy): eb has detected Y's fork, so the LowestAfter rule
    answers; with the fork column credited to X the unmarked entry of X sends
    the query to a HighestBefore entry that holds no seq."""
    sc = rd.get(name)
    diffs = rd.ancestry_diffs(sc)                            # (asserts the right map against the parent lists)
    assert diffs, "no observes() pair discriminates in %s" % name
    assert (sc.eb.id, sc.fy[0].id) in diffs
    on_fork = set(sc.fork_branch_ids)
    assert all(x in on_fork for _, x in diffs)


@pytest.mark.parametrize("name", NAMES)
def test_fork_evidence_needs_the_new_tables(name):
    V, X, Y, n, with_z, two = rd.VARIANTS[name]
    sc = rd.get(name)
    by_map, by_first = rd.fork_evidence_diffs(sc)            # (asserts the right tables against the naive rule)
    assert by_map, "no (head, creator) discriminates for fork evidence in %s" % name
    assert any(h == sc.eb.id and c == Y and stale == (0xFFFFFFFF, 0xFFFFFFFF, 0) for h, c, _, stale in by_map)
    assert all(c != X for _, c, _, _ in by_map)
    if [f.seq for f in sc.fx] != [f.seq for f in sc.fy] and by_first:
        assert all(right != stale for _, _, right, stale in by_first)
    # eb over P + A2 + T lists Y (and Z), never X
    seen = rd.cheaters_seen(sc, rd.kept(sc), [sc.eb])[sc.eb.id]
    assert Y in seen and X not in seen and (not with_z or sc.Z in seen)
    for e in rd.kept(sc):
        assert X not in rd.cheaters_seen(sc, rd.kept(sc), [e])[e.id]
    # the tables of A are warm with real content
    if n >= 24 or with_z:
        warm = rd.cheaters_seen(sc, sc.P + sc.A, sc.P + sc.A)
        assert any(warm.values()), name
        if n >= 24:
            assert any(X in s for s in warm.values()), name


def test_fork_evidence_first_seq_changes_in_a_two_variant():
    """Where the reused number's branch starts at another seq (W's fork in
    v5_two: seq 3 for X's 4), the right map with X's first seq gives other
    pairs."""
    names = [n for n in NAMES if rd.fork_evidence_diffs(rd.get(n))[1]]
    assert names and all(rd.VARIANTS[n][5] for n in names)


@pytest.mark.parametrize("name", NAMES)
def test_progress_pair_stakes_need_the_new_map(name):
    """Some event_progress pair stake differs with the fork column credited to
    X (beside the frames, which depend on Y's fork: rd.get(name, abft=True))."""
    sc = rd.get(name, abft=True)
    diffs = rd.progress_diffs(sc)
    assert diffs, "no event_progress pair stake discriminates in %s" % name
    assert all(a != b for _, _, a, b in diffs)


def test_reader_share():
    """The share the readers' GPU tests rest on: every reader discriminates in
    at least seven of the nine variants, the per-event cadence and a ``two``
    variant among them.  (All nine do; the tests above say which would not.)"""
    for reader in rd.READERS:
        ok = [n for n in NAMES if rd.reader_diffs(n)[reader]]
        assert len(ok) >= 7, (reader, ok)
        assert "v4_y_below" in ok and any(rd.VARIANTS[n][5] for n in ok), (reader, ok)


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
