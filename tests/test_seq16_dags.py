"""The two-speed DAGs of tests/seq16_dags.py meet, on the CPU oracles, the
conditions the GPU tests of the 16-bit seq boundary rest on: valid input,
max_seq exactly the intended value, ForklessCause answers that are a real mix,
an abft epoch that decides blocks.  A drifting generator fails here."""

import numpy as np
import pytest

from oracle import corc
import seq16_dags as sd

F, EVERY, SEED = 2, 64, 5
SPAN = {24: 512, 12: 256}        # as tests/test_gpu_seq16_boundary.py
MARKER = bytes(4) + (0x7FFFFFFF).to_bytes(4, "little")


def hb_max_seq(o, n):
    _, buf = o.rows(0, np.arange(n - 64, n, dtype=np.uint32))
    ent = buf.view(np.uint32).reshape(-1, 2)
    return int(ent[ent[:, 1] != 0x7FFFFFFF, 0].max())


@pytest.mark.parametrize("L", [sd.L_LAST16, sd.L_FIRST32, sd.L_CROSS], ids=hex)
@pytest.mark.parametrize("V", [24, 12])
def test_two_speed_shapes(V, L):
    d = sd.two_speed(V, F, L, EVERY, SEED)
    n = len(d)
    assert n == sd.level_end(d, L) == F * L + (V - F) * (L // EVERY)
    assert int((d.creator == 0).sum()) == L >= 0xFFFF
    # parents: self-parent first, distinct creators, older events
    cnt = np.diff(d.poff).astype(np.int64)
    assert cnt.max() <= 5 and np.all(d.par < np.repeat(np.arange(n), cnt))
    first = d.poff[:-1][cnt > 0].astype(np.int64)
    has = np.flatnonzero(cnt > 0)
    sp_ok = (d.creator[d.par[first]] == d.creator[has]) | (d.seq[has] == 1)
    assert sp_ok.all()
    for e in (n - 1, n // 2, sd.level_end(d, EVERY + 1) - 1):
        cs = d.creator[d.par[int(d.poff[e]):int(d.poff[e + 1])]]
        assert len(set(cs.tolist())) == len(cs)
    o = corc.OracleIndex(sd.SMALL_W[V])
    assert o.add_batch(d.creator, d.seq, d.poff, d.par) == -1
    assert o.num_branches() == V
    assert int(d.seq.max()) == L == hb_max_seq(o, n)
    qa, qb = sd.queries(n, 100_000, SPAN[V], seed=L)
    assert sd.fc_mix_ok(o.forkless_cause_batch(qa, qb))
    # a prefix cut at a level is a valid epoch with that max_seq and its own mix
    for cut in (sd.CUT_BEFORE, min(L, sd.L_LAST16)):
        n1 = sd.level_end(d, cut)
        o1 = corc.OracleIndex(sd.SMALL_W[V])
        assert o1.add_batch(d.creator[:n1], d.seq[:n1], d.poff[:n1 + 1], d.par) == -1
        assert int(d.seq[:n1].max()) == cut == hb_max_seq(o1, n1)
        qa, qb = sd.queries(n1, 100_000, SPAN[V], seed=cut)
        assert sd.fc_mix_ok(o1.forkless_cause_batch(qa, qb))


def test_two_speed_far_length():
    test_two_speed_shapes(24, sd.L_FAR)


@pytest.mark.parametrize("V", [24, 12])
def test_two_speed_fork_is_observed(V):
    d = sd.two_speed(V, F, sd.L_CROSS, EVERY, SEED, fork=True)
    plain = sd.two_speed(V, F, sd.L_CROSS, EVERY, SEED)
    assert len(d) == len(plain) + 1
    o = corc.OracleIndex(sd.SMALL_W[V])
    assert o.add_batch(d.creator, d.seq, d.poff, d.par) == -1
    assert o.num_branches() == V + 1
    n = len(d)
    assert o.merged_hb(n - 1)[8 * (V - 1):8 * V] == MARKER     # the newest event sees V-1 as a cheater
    assert hb_max_seq(o, n) == sd.L_CROSS
    qa, qb = sd.queries(n, 100_000, SPAN[V], seed=1)
    assert sd.fc_mix_ok(o.forkless_cause_batch(qa, qb))


def test_two_speed_other_continuation():
    V = 24
    a = sd.two_speed(V, F, sd.L_CROSS, EVERY, SEED)
    b = sd.two_speed(V, F, sd.L_LAST16, EVERY, SEED + 1, base=a, base_level=sd.CUT_BEFORE)
    n0 = sd.level_end(a, sd.CUT_BEFORE)
    assert sd.level_end(b, sd.CUT_BEFORE) == n0 and int(b.seq.max()) == sd.L_LAST16
    for x in ("creator", "seq", "lamport", "level"):
        assert np.array_equal(getattr(a, x)[:n0], getattr(b, x)[:n0])
    assert np.array_equal(a.par[:int(a.poff[n0])], b.par[:int(b.poff[n0])])
    nb = len(b)
    assert not np.array_equal(a.par[int(a.poff[n0]):int(a.poff[nb])], b.par[int(b.poff[n0]):int(b.poff[nb])])
    o = corc.OracleIndex(sd.SMALL_W[V])
    assert o.add_batch(b.creator, b.seq, b.poff, b.par) == -1


@pytest.mark.parametrize("wide", [False, True], ids=["small_w", "wide_w"])
def test_two_speed_abft_decides_blocks(wide):
    V = 24
    d = sd.two_speed(V, F, sd.L_CROSS, EVERY, SEED)
    a = corc.AbftOracle((sd.WIDE_W if wide else sd.SMALL_W)[V])
    rc, consumed, frames = a.process_batch(d.creator, d.seq, d.poff, d.par)
    assert rc == 0 and consumed == len(d)
    assert len(a.blocks) >= 100 and int(frames.max()) >= 100
