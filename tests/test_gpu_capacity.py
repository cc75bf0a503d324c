"""Every way a handle's device buffers grow, shrink and go away, while they
hold data (run on an MI355X: pytest -m gpu).

One handle is grown past its first event, seq, branch and local-column
capacities, reset across layouts, and created and destroyed many times.  Rows,
BranchesInfo and ForklessCause are compared with the C oracle as in
test_gpu_parity.py; that each path was taken is read from the handle's own
reports (device_bytes, branches_info, the stride of device_planes).  The
footprints are fixed by the growth policy (1.5x / 4096 events, 1.25x rounded to
64 branches, 1.5x / 256 seqs, 1.25x rounded to 16 local columns), not measured.
The constants below were recorded by running this file on the commit before the
buffers got an owning type (it uses the public API only): the footprint must
not move with a refactor of the handle's memory.
"""

import numpy as np
import pytest

from oracle import corc

pytestmark = pytest.mark.gpu

# device_bytes() as (planes, receive, per_event, other) after each stage
FOOTPRINT = {
    # after reset, after each of the five batches, after the drop, after the re-add
    "grow": [(2097152, 0, 98304, 66816), (2097152, 0, 98304, 66816), (4194304, 0, 98304, 133632),
             (4194304, 0, 98304, 133632), (6291456, 0, 147456, 133632), (6291456, 0, 147456, 199168),
             (6291456, 0, 147456, 199168), (6291456, 0, 147456, 199168)],
    # the same with option small_max=0: every batch through the device-assigned path, whose batch
    # scratch (ensure_batch, the scan scratch) and LowestAfter tail tables show in the last word
    "grow_big": [(2097152, 0, 98304, 66816), (2097152, 0, 98304, 149260), (4194304, 0, 98304, 331468),
                 (4194304, 0, 98304, 337228), (6291456, 0, 147456, 337228), (6291456, 0, 147456, 402764),
                 (6291456, 0, 147456, 402764), (6291456, 0, 147456, 402764)],
    # after the batch of each epoch
    "reset": [(4194304, 0, 98304, 526848), (12582912, 0, 98304, 1580544), (4194304, 0, 98304, 526848),
              (4194304, 0, 98304, 526848)],
    # shard 0, shard 1: after reset, after each of the two batches, after the exchange
    "shards": [(9437184, 0, 98304, 263424), (9437184, 0, 98304, 263424), (9437184, 0, 98304, 313100),
               (9437184, 0, 98304, 313100), (14155776, 0, 98304, 313100), (9437184, 0, 98304, 313100),
               (14155776, 0, 98304, 313100), (9437184, 0, 98304, 313100)],
}


@pytest.fixture(scope="module")
def lx():
    import lachesis_hip
    return lachesis_hip


def foot(ix):
    b = ix.device_bytes()
    return (b["planes"], b["receive"], b["per_event"], b["other"])


def compare_rows(ix, o, n):
    ev = np.arange(n, dtype=np.uint32)
    for mode in (0, 1):
        goff, gbuf = ix.rows_np(mode, ev)
        eoff, ebuf = o.rows(mode, ev)
        np.testing.assert_array_equal(goff, eoff)
        np.testing.assert_array_equal(gbuf, ebuf)


def compare_branches(ix, o, d, n):
    """branches_info against the oracle's branch of every event."""
    B = o.num_branches()
    last, creator = np.zeros(B, dtype=np.uint32), np.arange(B, dtype=np.uint32)
    for i in range(n):
        b = o.branch(i)
        creator[b] = d.creator[i]
        last[b] = max(last[b], d.seq[i])
    ls, cr = ix.branches_info()
    assert len(ls) == B
    has = last > 0                       # (a fork branch exists from its first event on)
    np.testing.assert_array_equal(ls, last)
    np.testing.assert_array_equal(cr[has], creator[has])
    return ls


def compare_fc(lx, ix, o, d, n, seed):
    qa, qb = lx.tools.fc_queries(d.lamport[:n], 20_000, window=24, seed=seed)
    np.testing.assert_array_equal(ix.forkless_cause_batch(qa, qb), o.forkless_cause_batch(qa, qb))


GROW_DAG = (20, 300, 4, 12, 8, 21)       # nodes, events/node, parents, cheaters, forks, seed
GROW_CUTS = [0, 120, 1500, 3000, 4500, 6000]
GROW_FLUSH = 3000


@pytest.mark.parametrize("path", ["small", "big"])
def test_one_handle_grown_every_way(lx, path):
    """event_capacity=64, branch_reserve=1: 4096 events, 256 seqs per branch
    and 64 branches at first; 6000 events of 20 validators with 12 cheaters pass
    all three while the handle holds rows.  Batches of at most 2048 events take
    the small-batch path by default; "big" (small_max=0) sends them through
    add_batch_dev, which also sizes the batch scratch and the tail tables."""
    n, ev, p, ch, fk, seed = GROW_DAG
    d = lx.tools.gen_dag(n, ev, p, ch, fk, seed)
    w = [1 + (i % 5) for i in range(n)]
    ix = lx.Index(event_capacity=64, branch_reserve=1, options={"small_max": 0} if path == "big" else None)
    ix.reset(w)
    o = corc.OracleIndex(w)
    stages = [foot(ix)]
    assert ix.device_planes()[2] == 64
    assert stages[0][2] == 6 * 4 * 4096          # the six per-event arrays at the first event capacity
    for lo, hi in zip(GROW_CUTS, GROW_CUTS[1:]):
        ix.add_batch(*d.slice(lo, hi))
        assert o.add_batch(*d.slice(lo, hi)) == -1
        if hi == GROW_FLUSH:
            ix.flush()
            o.flush()
        stages.append(foot(ix))
    N = len(d)
    assert ix.num_events() == N
    compare_rows(ix, o, N)
    ls = compare_branches(ix, o, d, N)
    compare_fc(lx, ix, o, d, N, seed)
    assert stages[-1][2] >= 6 * 4 * 6000 > stages[0][2]       # events grew
    assert int(ls.max()) > 256                                # seqs past the first s_cap
    assert ix.num_branches() > 64 and ix.device_planes()[2] >= ix.num_branches()   # branches past the first stride
    assert stages[1][0] > stages[0][0] or stages[2][0] > stages[0][0]
    # back to the flushed prefix, and forward again
    ix.drop_not_flushed()
    o.drop_not_flushed()
    assert ix.num_events() == GROW_FLUSH
    compare_rows(ix, o, GROW_FLUSH)
    compare_branches(ix, o, d, GROW_FLUSH)
    compare_fc(lx, ix, o, d, GROW_FLUSH, seed + 1)
    stages.append(foot(ix))
    for lo, hi in ((3000, 4500), (4500, 6000)):
        ix.add_batch(*d.slice(lo, hi))
        assert o.add_batch(*d.slice(lo, hi)) == -1
    compare_rows(ix, o, N)
    compare_branches(ix, o, d, N)
    compare_fc(lx, ix, o, d, N, seed + 2)
    stages.append(foot(ix))
    key = "grow" if path == "small" else "grow_big"
    print("FOOTPRINT", key, stages)
    ix.close()
    if path == "big":
        assert stages[-1][3] > FOOTPRINT["grow"][-1][3]          # batch scratch and tail tables are counted
    assert stages == FOOTPRINT[key]


RESET_SHAPES = [(20, 10, 4, 2, 3, 7), (300, 3, 5, 4, 2, 5), (8, 20, 3, 2, 3, 6), (8, 20, 3, 2, 3, 8)]


def test_reset_across_layouts(lx):
    """V = 20, 300 (re-layout up), 8 (more than 2x smaller: re-layout down), 8
    (steady: the buffers stay) on one handle."""
    ix = lx.Index()
    stages, strides = [], []
    for shape in RESET_SHAPES:
        n, ev, p, ch, fk, seed = shape
        d = lx.tools.gen_dag(n, ev, p, ch, fk, seed)
        w = [1 + (i % 4) for i in range(n)]
        ix.reset(w)
        ix.add_batch(d.creator, d.seq, d.poff, d.par)
        o = corc.OracleIndex(w)
        assert o.add_batch(d.creator, d.seq, d.poff, d.par) == -1
        compare_rows(ix, o, len(d))
        compare_branches(ix, o, d, len(d))
        compare_fc(lx, ix, o, d, len(d), seed)
        stages.append(foot(ix))
        strides.append(ix.device_planes()[2])
    print("FOOTPRINT reset", stages, strides)
    ix.close()
    assert strides == [128, 384, 128, 128]
    assert stages[1] != stages[0] and stages[1][0] > stages[0][0]
    assert stages[2] != stages[1] and stages[2][0] < stages[1][0]
    assert stages[3] == stages[2]
    assert stages == FOOTPRINT["reset"]


SHARD_DAG = (16, 40, 4, 8, 6, 31)
SHARD_CUTS = [0, 64, 640]          # shard 0 holds 22 columns after 64 events, 38 at the end


def shard_rows(shards, mode, ev):
    """What ShardedIndex.get_rows_dev's sum and max over the ranks do."""
    import torch
    dev = torch.device("cuda", 0)
    n = len(ev)
    slot = (shards[0].row_bytes_max() + 15) // 16 * 16
    t_ev = torch.from_numpy(ev.view(np.int32)).to(dev)
    total = torch.zeros(n * slot // 4, dtype=torch.int32, device=dev)
    length = torch.zeros(n, dtype=torch.int64, device=dev)
    for ix in shards:
        rows = torch.zeros(n * slot // 4, dtype=torch.int32, device=dev)
        lens = torch.zeros(n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        ix.get_rows_dev(mode, n, t_ev.data_ptr(), rows.data_ptr(), slot, lens.data_ptr())
        ix.sync()
        total += rows
        length = torch.maximum(length, lens.long() & 0xFFFFFFFF)
    rows, length = total.view(torch.uint8).view(n, slot).cpu().numpy(), length.cpu().numpy()
    return [bytes(rows[i, :int(k)]) for i, k in enumerate(length)]


def test_column_shards_grow_local_columns(lx):
    """G = 2 on one GPU: the eight cheaters are all creators of shard 0, whose
    plane columns pass its first local capacity (32) while it holds rows."""
    from test_gpu_shards import exchange, fc
    n, ev, p, ch, fk, seed = SHARD_DAG
    d = lx.tools.gen_dag(n, ev, p, ch, fk, seed)
    w = [1 + (i % 5) for i in range(n)]
    o = corc.OracleIndex(w)
    assert o.add_batch(d.creator, d.seq, d.poff, d.par) == -1
    shards = [lx.Index(branch_reserve=1, shard_rank=r, shard_count=2) for r in range(2)]
    stages = []
    for ix in shards:
        ix.reset(w)
        stages.append(foot(ix))
    assert [ix.device_planes()[2] for ix in shards] == [32, 32]
    for lo, hi in zip(SHARD_CUTS, SHARD_CUTS[1:]):
        for ix in shards:
            ix.add_batch(*d.slice(lo, hi))
            stages.append(foot(ix))
    assert shards[0].shard_range(0) == (0, 8)
    assert stages[2][0] == stages[0][0] < stages[4][0]        # shard 0's planes grew in the second batch, over 64 rows
    assert shards[0].device_planes()[2] > 32 and shards[1].device_planes()[2] == 32
    exchange(shards)
    for ix in shards:
        stages.append(foot(ix))
    qa, qb = lx.tools.fc_queries(d.lamport, 20_000, window=24, seed=seed)
    np.testing.assert_array_equal(fc(lx, shards, qa, qb), o.forkless_cause_batch(qa, qb))
    full = lx.Index()
    full.reset(w)
    full.add_batch(d.creator, d.seq, d.poff, d.par)
    evs = np.arange(len(d), dtype=np.uint32)
    for mode, get in ((0, full.highest_before_batch), (1, full.lowest_after_batch)):
        assert shard_rows(shards, mode, evs) == get(evs)
    print("FOOTPRINT shards", stages)
    for ix in shards + [full]:
        ix.close()
    assert stages == FOOTPRINT["shards"]


def test_no_leak_across_handles(lx):
    """Twenty handles created, filled and destroyed after a warm-up cycle: free
    device memory falls by no more than one handle's footprint (a leaked
    handle would cost twenty), and live_handles returns to where it was."""
    import torch
    n, ev, p, ch, fk, seed = GROW_DAG
    d = lx.tools.gen_dag(n, ev, p, ch, fk, seed)
    w = [1 + (i % 5) for i in range(n)]
    probe = lx.Index()
    live0 = probe.live_handles()

    def cycle():
        ix = lx.Index(event_capacity=64, branch_reserve=1)
        ix.reset(w)
        ix.add_batch(*d.slice(0, GROW_CUTS[1]))
        ix.add_batch(*d.slice(GROW_CUTS[1], GROW_CUTS[2]))
        ix.sync()
        total = ix.device_bytes()["total"]
        ix.close()
        return total

    one = cycle()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(0)[0]
    for _ in range(20):
        assert cycle() == one
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info(0)[0]
    print("LEAK one handle %d B, free before %d after %d" % (one, free0, free1))
    assert free0 - free1 <= one
    assert probe.live_handles() == live0
    probe.close()


LIFE_DAG = (4, 40, 2, 0, 0, 17)          # V = 4, two parents: 160 events
LIFE_BIG = 128                           # the smallest batch option segments = 2 splits (64 events per segment)
LX_ERR_ARG = -1


def test_handles_destroyed_with_every_lazy_resource_alive(lx):
    """Twenty handles created, driven and destroyed while each holds everything
    a handle makes on demand: a staging slot and its event (a batch through the
    walker), the segment events (option segments = 2), the resident row server
    and its stream (get_server = 2), the ForklessCause cache (one cached pair),
    the pinned query buffer (a per-call batch) and a pending small-path run.
    Destroying a handle with work pending is ordinary use: lx_destroy waits for
    it.  Device memory free after the twentieth cycle is not lower than after
    the second by more than one cycle's footprint (one buffer leaked per cycle
    would show eighteen times over), live_handles returns to its start after
    every destroy, a refused lx_create leaves it alone, and every answer on
    the way is the oracle's."""
    import torch
    n, ev, p, ch, fk, seed = LIFE_DAG
    d = lx.tools.gen_dag(n, ev, p, ch, fk, seed)
    w = [3, 2, 2, 1]
    o = corc.OracleIndex(w)                                        # as the index is after the walker's batch
    assert o.add_batch(*d.slice(0, LIFE_BIG)) == -1
    qa, qb = lx.tools.fc_queries(d.lamport[:LIFE_BIG], 500, window=24, seed=seed)
    fc_want = o.forkless_cause_batch(qa, qb)
    pair = (LIFE_BIG - 1, 3)
    pair_want = bool(o.forkless_cause_batch(np.array(pair[:1], np.uint32), np.array(pair[1:], np.uint32))[0])
    hb_last, la_5 = o.hb(LIFE_BIG - 1), o.la(5)
    assert o.add_batch(*d.slice(LIFE_BIG, LIFE_BIG + 1)) == -1
    hb_small = o.hb(LIFE_BIG)
    L = lx.load_library()
    live0 = L.lx_live_handles()

    with pytest.raises(lx.LxError) as refused:
        lx.Index(shard_rank=2, shard_count=2)
    assert refused.value.code == LX_ERR_ARG and L.lx_live_handles() == live0

    def free():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info(0)[0]

    def cycle(measure):
        before = free() if measure else 0
        ix = lx.Index(options={"small_max": 64, "segments": 2, "get_server": 2})
        assert L.lx_live_handles() == live0 + 1
        ix.reset(w)
        ix.add_batch(*d.slice(0, LIFE_BIG))                        # the walker path, as two segments
        assert ix.segment_stats()["segments"] == 2
        assert ix.highest_before(LIFE_BIG - 1) == hb_last     # one row, through the row server
        assert ix.lowest_after(5) == la_5
        srv = ix.get_server_stats()
        assert srv["launches"] >= 1 and srv["served"] >= 1
        assert ix.forkless_cause(*pair) == pair_want               # the result cache
        assert ix.forkless_cause(*pair) == pair_want and ix.fc_cache_stats()["hits"] >= 1
        np.testing.assert_array_equal(ix.forkless_cause_batch(qa, qb), fc_want)   # the pinned query buffer
        ix.add_batch(*d.slice(LIFE_BIG, LIFE_BIG + 1))             # the small path: pending until something reads
        assert ix.highest_before(LIFE_BIG) == hb_small
        ix.add_batch(*d.slice(LIFE_BIG + 1, LIFE_BIG + 2))         # ... and this one still is at the destroy
        assert ix.num_events() == LIFE_BIG + 2
        alive = free() if measure else 0
        ix.close()
        assert L.lx_live_handles() == live0
        return before - alive

    cycle(False)
    footprint = cycle(True)
    free2 = free()
    for _ in range(18):
        cycle(False)
    free20 = free()
    print("LIFECYCLE footprint %d B, free after cycle 2 %d, after cycle 20 %d" % (footprint, free2, free20))
    assert footprint > 0
    assert free2 - free20 <= footprint
