"""The 16-bit seq boundary (max_seq 0xFFFF / 0x10000) on every path that
``max_seq <= 0xFFFF`` switches: the walker's packed slot units and 8- / 12-column
slices, compact records, the small-batch kernels, rollback, the per-pair
ForklessCause cache (k_root_fc16 / k_root_fc), the abft engine's root-FC
kernels, the column shards' wire width and lx_load_rows.

Inputs are the two-speed DAGs of tests/seq16_dags.py (one creator really has
65,536 events), epochs of 0xFFFF, 0x10000 and 0x10028 levels, whole or cut at
level 0xFFFF (the handle sits at max_seq == 0xFFFF exactly, then crosses) or at
level 0xFFC0 (a batch crosses inside itself).  Everything is compared with the
C oracle: rows of every event in bulk, merged rows and branch ids on a sample,
100k ForklessCause answers.  Every case first asserts on the oracle's side
that add_batch accepted the input, that max_seq is the intended value and that
the ForklessCause answers are a real mix of true and false.

Durations on an MI355X (--durations=0, one process per test function, so the
first case of each function also builds its DAGs and oracles; seconds, the
slower of two runs):

  test_epoch_ends_at_boundary (16 cases)        first 9.8 (three DAGs, library load; 2.2 in the other run), cpw=1 at 0xFFFF 1.4, others 0.09-0.36
  test_epoch_ends_at_boundary_forked (3)        first 2.3, others 0.14-0.24
  test_crossing_between_batches (16)            first 2.6, others 0.19-0.29
  test_crossing_between_batches_forked (3)      first 2.3, others 0.18-0.22
  test_small_paths_cross_boundary (2)           V=12 4.2, V=24 0.7
  test_rollback_across_boundary (2)             default 3.6, cpw=12 0.6
  test_per_pair_fc_across_boundary (2)          small weights 2.6, wide 0.2
  test_abft_across_boundary (16)                first 4.1 (abft oracle 1 s), computed frames 1.1-2.8, claimed frames 0.09-0.18
  test_abft_root_pairs_per_pair_fc (6)          first 2.8, others 0.4-0.7
  test_shard_wire_changes_width (3)             first 3.3, others 0.3-0.6
  test_restart_at_boundary (1)                  3.3

No case exceeds 10 s, so every combination of walker variants and abft options
is kept; cpw=12,crec=1 is among the variants because compact records are off
by default.

What the cases catch was tried once with a library whose gates in
lx_fccache.cpp:283 and lx_index_shard.cpp:112 read 0x1FFFF (k_root_fc16 and the
uint16 wire past 16 bits, both read-only on their inputs):
test_per_pair_fc_across_boundary and test_shard_wire_changes_width failed,
test_abft_root_pairs_per_pair_fc did not -- the truncated compare is only
wrong for a pair whose HighestBefore entry lies above 0xFFFF and whose
LowestAfter entry below, on the two fast columns (6 of 28 stake), and no pair
of adjacent frames' roots is that close to the quorum.
"""

import numpy as np
import pytest

from oracle import corc
import seq16_dags as sd
from seq16_dags import CUT_BEFORE, L_CROSS, L_FAR, L_FIRST32, L_LAST16, level_end
from test_gpu_shards import exchange, fc

pytestmark = pytest.mark.gpu

F, EVERY, SEED = 2, 64, 5
SPAN = {24: 512, 12: 256}
NQ = 100_000


@pytest.fixture(scope="module")
def lx():
    import lachesis_hip
    return lachesis_hip


@pytest.fixture
def opts(monkeypatch):
    """Set lx_set_option values for every Index this test creates."""
    from lachesis_hip import capi

    def set_(**kw):
        for k, v in kw.items():
            monkeypatch.setitem(capi.DEFAULT_OPTIONS, k, v)
    return set_


class World:
    """DAGs, oracles and the oracles' rows, each built once per module and
    never modified afterwards."""

    def __init__(self):
        self._dag, self._orc, self._rows, self._abft = {}, {}, {}, {}

    def dag(self, V, L, fork=False):
        k = (V, L, fork)
        if k not in self._dag:
            self._dag[k] = sd.two_speed(V, F, L, EVERY, SEED, fork=fork)
        return self._dag[k]

    def oracle(self, V, L, fork=False, upto=None, wide=False):
        """Oracle over the events up to level ``upto`` (default: all) of the
        epoch of L levels; asserts the oracle-side input conditions."""
        upto = L if upto is None else upto
        k = (V, L, fork, upto, wide)
        if k not in self._orc:
            d = self.dag(V, L, fork)
            n = level_end(d, upto)
            o = corc.OracleIndex((sd.WIDE_W if wide else sd.SMALL_W)[V])
            assert o.add_batch(d.creator[:n], d.seq[:n], d.poff[:n + 1], d.par) == -1
            assert oracle_max_seq(o, n) == upto == int(d.seq[:n].max())
            assert o.num_branches() == V + (1 if fork else 0)
            self._orc[k] = o
        return self._orc[k]

    def rows(self, o, mode, lo, hi):
        k = (id(o), mode, lo, hi)
        if k not in self._rows:
            self._rows[k] = o.rows(mode, np.arange(lo, hi, dtype=np.uint32))
        return self._rows[k]

    def abft(self, V, L, wide):
        k = (V, L, wide)
        if k not in self._abft:
            d = self.dag(V, L)
            a = corc.AbftOracle((sd.WIDE_W if wide else sd.SMALL_W)[V])
            rc, consumed, frames = a.process_batch(d.creator, d.seq, d.poff, d.par)
            assert rc == 0 and consumed == len(d)
            assert len(a.blocks) >= 100
            self._abft[k] = (a, frames)
        return self._abft[k]


@pytest.fixture(scope="module")
def world():
    return World()


def oracle_max_seq(o, n):
    """The largest seq the oracle's HighestBefore rows of the last events hold."""
    _, buf = o.rows(0, np.arange(max(0, n - 64), n, dtype=np.uint32))
    ent = buf.view(np.uint32).reshape(-1, 2)
    return int(ent[ent[:, 1] != 0x7FFFFFFF, 0].max())


ROW_CHUNK = 40_000


def check_all_rows(world, ix, o, n):
    """HighestBefore and LowestAfter of every event 0..n-1, byte for byte."""
    for mode in (0, 1):
        for lo in range(0, n, ROW_CHUNK):
            hi = min(n, lo + ROW_CHUNK)
            eoff, ebuf = world.rows(o, mode, lo, hi) if world else o.rows(mode, np.arange(lo, hi, dtype=np.uint32))
            goff, gbuf = ix.rows_np(mode, np.arange(lo, hi, dtype=np.uint32))
            if not (np.array_equal(goff, eoff) and np.array_equal(gbuf, ebuf)):
                bad = first_bad_row(goff, gbuf, eoff, ebuf)
                raise AssertionError("mode %d: row of event %d differs: got %s, oracle %s" % (
                    mode, lo + bad, gbuf[int(goff[bad]):int(goff[bad + 1])].tobytes().hex(),
                    ebuf[int(eoff[bad]):int(eoff[bad + 1])].tobytes().hex()))


def first_bad_row(goff, gbuf, eoff, ebuf):
    for i in range(len(eoff) - 1):
        if gbuf[int(goff[i]):int(goff[i + 1])].tobytes() != ebuf[int(eoff[i]):int(eoff[i + 1])].tobytes():
            return i
    return len(eoff) - 2


def check_rows_of(ix, o, evs):
    evs = np.ascontiguousarray(evs, dtype=np.uint32)
    for mode in (0, 1):
        eoff, ebuf = o.rows(mode, evs)
        goff, gbuf = ix.rows_np(mode, evs)
        if not (np.array_equal(goff, eoff) and np.array_equal(gbuf, ebuf)):
            raise AssertionError("mode %d: row of event %d differs" % (mode, int(evs[first_bad_row(goff, gbuf, eoff, ebuf)])))


def sample_events(d, n, seed, from_level=CUT_BEFORE):
    """2000 random events of the first n plus every event of level >= from_level."""
    rng = np.random.default_rng(seed)
    lo = min(n, level_end(d, from_level - 1)) if from_level <= len(d.level_ends) else n
    return np.unique(np.concatenate([rng.choice(n, min(n, 2000), replace=False), np.arange(lo, n)])).astype(np.uint32)


def check_merged_and_branch(ix, o, evs):
    got = ix.merged_highest_before_batch(evs)
    for k, e in enumerate(evs):
        e = int(e)
        assert got[k] == o.merged_hb(e), ("merged", e)
        assert ix.branch(e) == o.branch(e), ("branch", e)


def fc_set(o, n, V, seed):
    """100k queries over the first n events and the oracle's answers (a real
    mix, over all queries and over the tail half)."""
    qa, qb = sd.queries(n, NQ, SPAN[V], seed)
    exp = o.forkless_cause_batch(qa, qb)
    assert sd.fc_mix_ok(exp), (float(exp.mean()), float(exp[NQ // 2:].mean()))
    return qa, qb, exp


def check_fc(ix, o, n, V, seed):
    qa, qb, exp = fc_set(o, n, V, seed)
    np.testing.assert_array_equal(ix.forkless_cause_batch(qa, qb), exp)


def check_index(world, ix, o, d, n, V, seed):
    assert ix.num_events() == n == o.num_events()
    assert ix.num_branches() == o.num_branches()
    check_all_rows(world, ix, o, n)
    check_merged_and_branch(ix, o, sample_events(d, n, seed))
    check_fc(ix, o, n, V, seed)


def add(ix, d, lo, hi):
    ix.add_batch(d.creator[lo:hi], d.seq[lo:hi], d.poff[lo:hi + 1], d.par)


# walker variants: {} takes side-by-side segments at this size on its own;
# crec=1 streams the 32-byte compact records on the 8- / 12-column walks
VARIANTS = [{}, {"cpw": 1}, {"cpw": 4}, {"cpw": 4, "pack16": 0}, {"cpw": 8}, {"cpw": 12}, {"cpw": 12, "crec": 0},
            {"cpw": 12, "crec": 1}]
FORK_VARIANTS = [{}, {"cpw": 4}, {"cpw": 12}]
vid = lambda v: ",".join("%s=%s" % kv for kv in v.items()) or "default"


def new_index(lx, V, n, wide=False, **options):
    ix = lx.Index(event_capacity=n, options=options or None)
    ix.reset((sd.WIDE_W if wide else sd.SMALL_W)[V])
    return ix


# ------------------------------------------------ a / c: an epoch ending at the boundary, one batch
def one_batch(lx, world, opts, variant, L, fork):
    V = 24
    opts(small_max=0, **variant)
    d = world.dag(V, L, fork)
    o = world.oracle(V, L, fork)
    ix = new_index(lx, V, len(d))
    add(ix, d, 0, len(d))       # at L = 0x10000 the 8- / 12-column options fall back, no error
    check_index(world, ix, o, d, len(d), V, seed=L)
    ix.close()


@pytest.mark.parametrize("variant", VARIANTS, ids=vid)
@pytest.mark.parametrize("L", [L_LAST16, L_FIRST32], ids=hex)
def test_epoch_ends_at_boundary(lx, world, opts, variant, L):
    """The last packed epoch (0xFFFF sits in a 16-bit lane) and the first
    unpacked one, the whole epoch as one walker batch."""
    one_batch(lx, world, opts, variant, L, fork=False)


@pytest.mark.parametrize("variant", FORK_VARIANTS, ids=vid)
def test_epoch_ends_at_boundary_forked(lx, world, opts, variant):
    """B > V at max_seq 0x10000: the masked kernels, fork marks (bit 31) next
    to seqs above 0xFFFF, the wide-slice options falling back for two reasons."""
    one_batch(lx, world, opts, variant, L_FIRST32, fork=True)


# ------------------------------------------------ b / c: crossing between batches
def crossing(lx, world, opts, variant, cut, fork):
    V, L = 24, L_CROSS
    opts(small_max=0, **variant)
    d = world.dag(V, L, fork)
    o1 = world.oracle(V, L, fork, upto=cut)
    o = world.oracle(V, L, fork)
    n1, n = level_end(d, cut), len(d)
    ix = new_index(lx, V, n)
    add(ix, d, 0, n1)
    check_index(world, ix, o1, d, n1, V, seed=cut)
    add(ix, d, n1, n)
    # all rows: batch 2 has just written LowestAfter entries above 0xFFFF into batch 1's rows
    check_index(world, ix, o, d, n, V, seed=L)
    ix.close()


@pytest.mark.parametrize("variant", VARIANTS, ids=vid)
@pytest.mark.parametrize("cut", [L_LAST16, CUT_BEFORE], ids=hex)
def test_crossing_between_batches(lx, world, opts, variant, cut):
    """Cut at level 0xFFFF: the handle sits at max_seq == 0xFFFF exactly after
    batch 1, rows written by the packed kernels are read and joined by the
    unpacked ones.  Cut at 0xFFC0: batch 2 crosses inside itself."""
    crossing(lx, world, opts, variant, cut, fork=False)


@pytest.mark.parametrize("variant", FORK_VARIANTS, ids=vid)
def test_crossing_between_batches_forked(lx, world, opts, variant):
    crossing(lx, world, opts, variant, L_LAST16, fork=True)


# ------------------------------------------------ d: small and single-event paths across the boundary
D_PREFIX = 0xFE00    # the chunked remainder starts here (see test_small_paths_cross_boundary)


def chunk_plan(d, n0, n, seed):
    """Chunks [lo, hi) of events n0..n with seeded random sizes within 1..2048:
    single events, short runs (k_small) and runs >= 128 levels deep
    (k_small_dbl on few branches).  Only 40 levels lie above 0xFFFF, so the
    first seed from ``seed`` on is taken whose plan has every kind of chunk on
    both sides (plan_covers; a condition on the input alone)."""
    for s in range(seed, seed + 100_000, 100):
        rng = np.random.default_rng(s)
        out, lo = [], n0
        while lo < n:
            r = rng.random()
            size = 1 if r < 0.4 else int(rng.integers(2, 25)) if r < 0.75 else int(rng.integers(300, 420))
            out.append((lo, min(n, lo + size)))
            lo = out[-1][1]
        if plan_covers(d, out):
            return out
    raise AssertionError("no chunk plan covers both sides of the boundary")


def plan_covers(d, plan):
    """Single fast-validator events with seq below and above 0xFFFF; runs >= 128
    levels deep and shallower runs, each both ending at or below level 0xFFFF
    and reaching above it."""
    depth = lambda c: int(d.level[c[1] - 1]) - int(d.level[c[0]]) + 1
    below = lambda c: int(d.level[c[1] - 1]) <= 0xFFFF
    single = [c for c in plan if c[1] - c[0] == 1 and d.creator[c[0]] < F]
    deep = [c for c in plan if depth(c) >= 128]
    shallow = [c for c in plan if c[1] - c[0] > 1 and depth(c) < 128]
    return all(any(below(c) for c in kind) and any(not below(c) for c in kind) for kind in (single, deep, shallow))


@pytest.mark.parametrize("V", [12, 24])
def test_small_paths_cross_boundary(lx, world, V):
    """Host-pointer chunks on default options (k_small, k_small_dbl on V = 12,
    single events with the fused Add + cache-row launch k_add1_row) below, across
    and above seq 0xFFFF, after a walker batch; a walker-only scratch handle;
    on V = 12 a third handle with the whole epoch in 3000-event batches
    (k_dbl on both sides).

    The chunked remainder starts at level 0xFE00, not 0xFFC0: from 0xFFC0 only
    104 levels (~230 events) remain, so no run could be 128 levels deep, and
    one random chunk would swallow them all.  Each chunk is read back right
    away, so every chunk is a run of its own."""
    L = L_CROSS
    d = world.dag(V, L)
    o = world.oracle(V, L)
    n0, nc, n = level_end(d, D_PREFIX), level_end(d, CUT_BEFORE), len(d)
    plan = chunk_plan(d, n0, n, seed=V)
    assert plan_covers(d, plan) and max(hi - lo for lo, hi in plan) <= 2048

    scratch = new_index(lx, V, n, small_max=0)
    add(scratch, d, 0, nc)
    add(scratch, d, nc, n)

    ix = new_index(lx, V, n)
    add(ix, d, 0, n0)
    rng = np.random.default_rng(V)
    for lo, hi in plan:
        add(ix, d, lo, hi)
        e = hi - 1
        if hi - lo == 1:
            # the caller's Add-then-ForklessCause miss; the answer never changes later
            b = int(rng.integers(max(0, e - SPAN[V]), e))
            assert ix.forkless_cause(e, b) == bool(o.forkless_cause(e, b)), (e, b)
        assert ix.highest_before(e) == o.hb(e), e
    assert ix.fc_cache_stats()["row_fills"] > 0

    handles = [scratch, ix]
    if V == 12:
        dbl = new_index(lx, V, n, small_max=0, dbl=1)
        for lo in range(0, n, 3000):
            add(dbl, d, lo, min(n, lo + 3000))
        handles.append(dbl)
    ev = sample_events(d, n, seed=V, from_level=0xFF00)
    qa, qb, exp = fc_set(o, n, V, seed=V)
    for h in handles:
        assert h.num_events() == n and h.num_branches() == o.num_branches()
        check_rows_of(h, o, ev)
        check_merged_and_branch(h, o, ev[::4])
        np.testing.assert_array_equal(h.forkless_cause_batch(qa, qb), exp)
        h.close()


# ------------------------------------------------ e: rollback across the boundary
@pytest.mark.parametrize("variant", [{}, {"cpw": 12}], ids=vid)
def test_rollback_across_boundary(lx, world, opts, variant):
    """Flush at level 0xFFC0, add the crossing remainder, DropNotFlushed (the
    prefix's LowestAfter entries above 0xFFFF go away), add a different
    continuation that ends at level 0xFFFF, flush, cross again."""
    V = 24
    opts(small_max=0, **variant)
    dA = world.dag(V, L_CROSS)
    dB = sd.two_speed(V, F, L_LAST16, EVERY, SEED + 1, base=dA, base_level=CUT_BEFORE)
    dC = sd.two_speed(V, F, L_CROSS, EVERY, SEED + 2, base=dB, base_level=L_LAST16)
    n0, nA, nB, nC = level_end(dA, CUT_BEFORE), len(dA), len(dB), len(dC)
    assert np.array_equal(dB.par[:int(dB.poff[n0])], dA.par[:int(dA.poff[n0])])
    assert not np.array_equal(dB.par[int(dB.poff[n0]):int(dB.poff[nB])], dA.par[int(dA.poff[n0]):int(dA.poff[nB])])
    o = corc.OracleIndex(sd.SMALL_W[V])
    ix = new_index(lx, V, nC)

    def step(d, lo, hi, max_seq, seed):
        if hi > lo:
            assert o.add_batch(d.creator[lo:hi], d.seq[lo:hi], d.poff[lo:hi + 1], d.par) == -1
            add(ix, d, lo, hi)
        assert oracle_max_seq(o, hi) == max_seq
        check_index(None, ix, o, d, hi, V, seed)

    step(dA, 0, n0, CUT_BEFORE, 1)
    ix.flush()
    o.flush()
    step(dA, n0, nA, L_CROSS, 2)
    ix.drop_not_flushed()
    o.drop_not_flushed()
    step(dA, n0, n0, CUT_BEFORE, 3)
    step(dB, n0, nB, L_LAST16, 4)
    ix.flush()
    o.flush()
    step(dC, nB, nC, L_CROSS, 5)
    ix.close()


# ------------------------------------------------ f: per-pair lx_forkless_cause (result cache -> k_root_fc16 / k_root_fc)
def caller_pairs(d, n, V, seed, n_a=100, per_a=20):
    """Single pairs as abft asks them: a among the last 200 events, b among the
    slow validators' events and the fast validators' wide events (level = 1 mod
    every) within the query span before a."""
    rng = np.random.default_rng(seed)
    wide = (d.creator[:n] >= F) | (d.level[:n] % EVERY == 1)
    out = []
    for a in rng.choice(np.arange(n - 200, n), n_a, replace=False):
        cand = np.flatnonzero(wide[max(0, a - SPAN[V]):a + 1]) + max(0, a - SPAN[V])
        out += [(int(a), int(b)) for b in rng.choice(cand, min(per_a, len(cand)), replace=False)]
    return out


@pytest.mark.parametrize("wide", [False, True], ids=["small_w", "wide_w"])
def test_per_pair_fc_across_boundary(lx, world, wide):
    """lx_forkless_cause one pair at a time after the batch that ends at
    max_seq 0xFFFF (row fills by k_root_fc16; weights >= 2^16 take its
    high-half dot products) and after the crossing batch (k_root_fc); the
    answers given before the crossing are asked again after it."""
    V, L = 24, L_CROSS
    d = world.dag(V, L)
    o1 = world.oracle(V, L, upto=L_LAST16, wide=wide)
    o = world.oracle(V, L, wide=wide)
    n1, n = level_end(d, L_LAST16), len(d)
    ix = new_index(lx, V, n, wide=wide)
    add(ix, d, 0, n1)
    p1 = caller_pairs(d, n1, V, seed=1)
    exp1 = [bool(o1.forkless_cause(a, b)) for a, b in p1]
    assert len(p1) >= 2000 and 0.2 <= np.mean(exp1) <= 0.8, np.mean(exp1)
    for (a, b), e in zip(p1, exp1):
        assert ix.forkless_cause(a, b) == e, (a, b)
    st1 = ix.fc_cache_stats()
    assert st1["calls"] == len(p1) and st1["calls"] - st1["hits"] > 0 and st1["row_fills"] > 0, st1
    add(ix, d, n1, n)
    p2 = caller_pairs(d, n, V, seed=2)
    exp2 = [bool(o.forkless_cause(a, b)) for a, b in p2]
    assert len(p2) >= 2000 and 0.2 <= np.mean(exp2) <= 0.8, np.mean(exp2)
    for (a, b), e in zip(p2 + p1, exp2 + [bool(o.forkless_cause(a, b)) for a, b in p1]):
        assert ix.forkless_cause(a, b) == e, (a, b)
    assert [bool(o.forkless_cause(a, b)) for a, b in p1] == exp1
    st2 = ix.fc_cache_stats()
    assert st2["row_fills"] > st1["row_fills"] and st2["calls"] - st2["hits"] > st1["calls"] - st1["hits"], st2
    ix.close()


# ------------------------------------------------ g: abft across the boundary
def abft_run(d, weights, fc16, claims, cuts):
    from lachesis_hip import abft
    lch = abft.DenseLachesis(weights, event_capacity=len(d))
    lch.set_option("fc16", fc16)
    frames = np.zeros(len(d), dtype=np.uint32)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        if hi == lo:
            continue
        c, s, off, par = d.slice(lo, hi)
        rc, consumed, out = lch.process_batch(c, s, off, par, None if claims is None else claims[lo:hi])
        assert rc == 0 and consumed == hi - lo
        frames[lo:hi] = out
    return lch, frames


@pytest.mark.parametrize("wide", [False, True], ids=["small_w", "wide_w"])
@pytest.mark.parametrize("claimed", [0, 1])
@pytest.mark.parametrize("fc16", [1, 0])
@pytest.mark.parametrize("L", [L_LAST16, L_CROSS], ids=hex)
def test_abft_across_boundary(world, L, fc16, claimed, wide):
    """The abft engine on an epoch that ends at max_seq 0xFFFF or crosses it
    (its root-FC tiles change from k_root_fc16 to k_root_fc mid-epoch), one
    batch and chunks cut at levels 0xFFC0 and 0xFFFF: every event's frame, the
    roots of every frame and every block equal the C abft restatement's."""
    V = 24
    d = world.dag(V, L)
    world.oracle(V, L)            # max_seq and add_batch, asserted on the index oracle
    ref, ref_frames = world.abft(V, L, wide)
    weights = (sd.WIDE_W if wide else sd.SMALL_W)[V]
    n = len(d)
    n_frames = int(ref_frames.max())
    ref_roots = [set(map(int, ref.frame_roots(f))) for f in range(n_frames + 2)]
    for cuts in ([0, n], [0, level_end(d, CUT_BEFORE), level_end(d, L_LAST16), n]):
        lch, frames = abft_run(d, weights, fc16, ref_frames if claimed else None, cuts)
        assert np.array_equal(frames, ref_frames), cuts
        for f in range(n_frames + 2):
            assert set(map(int, lch.frame_roots(f))) == ref_roots[f], (cuts, f)
        assert lch.blocks == ref.blocks, cuts
        lch.close()


@pytest.mark.parametrize("wide", [False, True], ids=["small_w", "wide_w"])
@pytest.mark.parametrize("L", [L_LAST16, L_CROSS, L_FAR], ids=hex)
def test_abft_root_pairs_per_pair_fc(lx, world, L, wide):
    """What the block comparison cannot show: for the roots of the last 20
    frames, ForklessCause(e, r) of every successor-frame root e against every
    root r, asked of the per-pair lx_forkless_cause on an Index fed the same
    events in the same chunks, equals the index oracle's answer.  A frame
    spans ~160 levels, so at 0x10028 no root lies above the boundary yet; at
    0x10400 the roots of the last six frames do."""
    V = 24
    d = world.dag(V, L)
    o = world.oracle(V, L, wide=wide)
    ref, ref_frames = world.abft(V, L, wide)
    n = len(d)
    ix = new_index(lx, V, n, wide=wide)
    cuts = [0, level_end(d, CUT_BEFORE), level_end(d, L_LAST16), n]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        if hi > lo:
            add(ix, d, lo, hi)
    top = int(ref_frames.max())
    pairs = [(int(e), int(r)) for f in range(top - 20, top) for r in ref.frame_roots(f) for e in ref.frame_roots(f + 1)]
    exp = [bool(o.forkless_cause(e, r)) for e, r in pairs]
    # this set is given by the frames, not drawn: a root of frame f + 1 forkless-causes
    # roots of frame f holding more than 2/3 of the stake by definition, so well over
    # half of the answers are true; what the check needs is both answers in numbers
    assert len(pairs) >= 2000 and 0.1 <= np.mean(exp) <= 0.9, (len(pairs), np.mean(exp))
    assert int(d.seq[[e for e, _ in pairs]].max()) >= L - 2 * EVERY      # the pairs reach the end of the epoch
    if L == L_FAR:
        assert sum(1 for e, r in pairs if d.creator[r] < F and d.seq[r] > 0xFFFF) >= 100
    for (e, r), want in zip(pairs, exp):
        assert ix.forkless_cause(e, r) == want, (e, r)
    st = ix.fc_cache_stats()
    assert st["row_fills"] > 0 and st["calls"] - st["hits"] > 0, st
    ix.close()


# ------------------------------------------------ h: column shards change wire width between exchanges
@pytest.mark.parametrize("G,fork", [(2, False), (3, False), (2, True)])
def test_shard_wire_changes_width(lx, world, G, fork):
    V, L = 24, L_CROSS
    d = world.dag(V, L, fork)
    o1 = world.oracle(V, L, fork, upto=L_LAST16)
    o = world.oracle(V, L, fork)
    n1, n = level_end(d, L_LAST16), len(d)
    shards = []
    for r in range(G):
        ix = lx.Index(shard_rank=r, shard_count=G, event_capacity=n)
        ix.reset(sd.SMALL_W[V])
        add(ix, d, 0, n1)
        shards.append(ix)
    widths = exchange(shards)
    assert all(ix.shard_wire_bytes() == 2 for ix in shards)
    assert set(widths.values()) <= {1, 2}
    qa, qb, exp = fc_set(o1, n1, V, seed=G)
    np.testing.assert_array_equal(fc(lx, shards, qa, qb), exp)
    for ix in shards:
        add(ix, d, n1, n)
    widths = exchange(shards)
    assert all(ix.shard_wire_bytes() == 4 for ix in shards)
    assert set(widths.values()) <= {1, 4}
    qa, qb, exp = fc_set(o, n, V, seed=G + 10)
    np.testing.assert_array_equal(fc(lx, shards, qa, qb), exp)
    for ix in shards:
        ix.close()


# ------------------------------------------------ i: restart at the boundary
def test_restart_at_boundary(lx, world):
    """Tables written back at a flush at level 0xFFFF (the loaded handle must
    stay on the packed paths) and at level 0x10010 (it must not); each fresh
    handle, with option cpw=12, continues to 0x10028 and equals the oracle."""
    V, L = 24, L_CROSS
    d = world.dag(V, L)
    o = world.oracle(V, L)
    n = len(d)
    A = new_index(lx, V, n, small_max=0)
    tabs = {"S": {}, "s": {}, "b": {}}
    lo = 0
    loads = []
    for lvl in (L_LAST16, 0x10010):
        hi = level_end(d, lvl)
        add(A, d, lo, hi)
        wb = A.writeback()
        for t in tabs:
            tabs[t].update(wb[t])
        A.flush()
        loads.append((lvl, hi, {t: dict(tabs[t]) for t in tabs}, wb["B"]))
        lo = hi
    A.close()
    for lvl, cut, tb, bi in loads:
        o1 = world.oracle(V, L, upto=lvl)
        R = new_index(lx, V, n, small_max=0, cpw=12)
        R.load_rows(d.creator[:cut], d.seq[:cut], d.poff[:cut + 1], d.par, b"".join(tb["b"][k] for k in range(cut)),
                    [tb["S"][k] for k in range(cut)], [tb["s"][k] for k in range(cut)])
        R.load_finish(bi)
        check_all_rows(world, R, o1, cut)
        add(R, d, cut, n)
        check_index(world, R, o, d, n, V, seed=lvl)
        R.close()
