"""The early exit of batched ForklessCause in fork epochs (k_fc_fk_early,
option fc_early_forks; run on an MI355X: pytest -m gpu).

With the option on, an epoch of 1..64 cheaters and more than 512 validators
answers launches of >= 2^14 queries in rounds and stops a query once its count
decides the quorum.  The answers must equal the oracle's
(vecfc/forkless_cause.go:40-82) and, byte for byte, the whole-row kernel's;
the device's per-round counters must equal the model of
tests/fc_fork_directed.py (pinned to the oracle by
tests/test_fc_fork_directed_model.py); and an epoch or launch that misses one of
the gate's conditions must not take the path at all."""

import numpy as np
import pytest

import fc_directed as fd
import fc_fork_directed as ff
from oracle import corc
from test_gpu_fc_directed import write_rows

pytestmark = pytest.mark.gpu

ZERO = (0, 0, 0, 0)


@pytest.fixture(scope="module")
def lx():
    import lachesis_hip
    return lachesis_hip


def oracle_of(d, w):
    o = corc.OracleIndex(w)
    assert o.add_batch(d.creator, d.seq, d.poff, d.par) == -1
    return o


def index_of(lx, d, w, **options):
    ix = lx.Index(event_capacity=len(d), options=options)
    ix.reset(w)
    ix.add_batch(d.creator, d.seq, d.poff, d.par)
    ix.sync()
    return ix


def ask(ix, qa, qb):
    """(answers, fork-path counters, fork-free-path counters) of one launch."""
    ix.fc_early_fork_rounds()
    ix.fc_early_rounds()
    got = ix.forkless_cause_batch(qa, qb)
    return got, ix.fc_early_fork_rounds(), ix.fc_early_rounds()


def test_option_and_entry_point(lx):
    """The public surface: the option exists, takes 0 or 1 and is off by
    default; the counters read zero on a handle that never took the path."""
    ix = lx.Index()
    assert hasattr(ix.L, "lx_fc_early_fork_rounds")
    assert ix.fc_early_fork_rounds() == ZERO
    ix.set_option("fc_early_forks", 1)
    ix.set_option("fc_early_forks", 0)
    with pytest.raises(lx.capi.LxError):
        ix.set_option("fc_early_forks", 2)
    ix.close()


@pytest.mark.parametrize("name", list(ff.RANDOM_CASES))
def test_equals_oracle_and_whole_rows(lx, name):
    d, w, qa, qb = ff.random_case(name)
    V = ff.RANDOM_CASES[name][0]
    o = oracle_of(d, w)
    want = o.forkless_cause_batch(qa, qb)
    ix = index_of(lx, d, w)
    # off by default: whole rows
    whole, fork_rounds, rounds = ask(ix, qa, qb)
    assert fork_rounds == ZERO and rounds[0] == 0
    np.testing.assert_array_equal(whole, want)
    ix.set_option("fc_early_forks", 1)
    got, fork_rounds, rounds = ask(ix, qa, qb)
    print("%s: fork rounds %s of %d" % (name, fork_rounds, len(qa)))
    np.testing.assert_array_equal(got, want)
    assert got.tobytes() == whole.tobytes()
    assert fork_rounds[2] == len(qa) and fork_rounds[0] < fork_rounds[2]
    assert fork_rounds[3] <= fork_rounds[1] <= fork_rounds[0]
    assert rounds[0] == 0
    # the device stops every query where the model does
    hb, la, bc, branch = ff.oracle_planes(o, d, V)
    assert fork_rounds == ff.counters(ff.model(hb, la, bc, branch, w, qa, qb)["rnd"])
    ix.set_option("fc_early_forks", 0)
    again, fork_rounds, _ = ask(ix, qa, qb)
    assert fork_rounds == ZERO and again.tobytes() == whole.tobytes()
    ix.close()


N14 = ff.MIN_QUERIES


@pytest.mark.parametrize("name", list(ff.GATE_CASES))
def test_gate(lx, name):
    """Both sides of every condition of lx_fc_args' gate: the launches that miss
    one leave the fork path's counters at zero (a fork-free epoch runs
    k_fc_early instead), and every answer equals the oracle's."""
    options, n, fork_free_path = ff.GATE_CASES[name][5:]
    is_open = name in ff.GATE_OPEN
    d, w, qa, qb = ff.gate_case(name)
    o = oracle_of(d, w)
    B = o.num_branches()
    want = o.forkless_cause_batch(qa, qb)
    ix = index_of(lx, d, w, **dict({"fc_early_forks": 1}, **options))
    assert ix.num_branches() == B
    got, fork_rounds, rounds = ask(ix, qa, qb)
    np.testing.assert_array_equal(got, want)
    assert 0.05 < want.mean() < 0.95
    if is_open:
        assert fork_rounds[2] == n and fork_rounds[0] < n
    else:
        assert fork_rounds == ZERO
    assert rounds[0] == (n if fork_free_path else 0)
    ix.close()


def test_unknown_events(lx):
    """Queries on events past the index answer 0xFF through the fork path too,
    lx_sync reports the flag, and the counter shows every query took the path."""
    import torch
    V = 600
    d = ff.fork_dag(V, 12, 3, 3, False, seed=33)
    w = ff.zipf(V)
    ix = index_of(lx, d, w, fc_early_forks=1)
    assert ix.num_branches() > V
    dev = torch.device("cuda", 0)
    n = N14
    qa, qb = lx.tools.fc_queries(d.lamport, n, window=64, seed=5)
    qa[:3] = [0, len(d) + 5, 7]
    qb[:3] = [len(d) + 9, 1, 3]
    ta = torch.from_numpy(qa.view(np.int32)).to(dev)
    tb = torch.from_numpy(qb.view(np.int32)).to(dev)
    out = torch.zeros(n, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ix.fc_early_fork_rounds()
    ix.forkless_cause_batch_dev(n, ta.data_ptr(), tb.data_ptr(), out.data_ptr())
    with pytest.raises(Exception):
        ix.sync()                                        # the unknown-event flag is reported
    got = out.cpu().numpy()
    assert got[0] == 0xFF and got[1] == 0xFF and got[2] in (0, 1)
    np.testing.assert_array_equal(got[3:], oracle_of(d, w).forkless_cause_batch(qa[3:], qb[3:]))
    assert ix.fc_early_fork_rounds()[2] == n
    ix.close()


def test_directed_rows(lx):
    """Crafted rows over a real fork DAG's branch tables (V = 534: a straddling
    uint4; four cheaters with originals in rounds 2, 3, 4 and the straddling
    uint4): rows on count = quorum - 1 / quorum and count + rest = quorum - 1 /
    quorum in every round, cheaters counting through a fork branch only, the
    original only, both (once), marked (not at all), the early false over a
    count above the quorum, pad columns that would count.  All 65,536 pairs:
    the booleans and the four counters equal the model exactly."""
    d = ff.directed_dag()
    w = ff.directed_weights()
    Q = fd.quorum_of(w)
    ix = lx.Index(event_capacity=len(d), options={"fc_early_forks": 1})
    ix.reset(w)
    branch = ix.add_batch(d.creator, d.seq, d.poff, d.par, want_branches=True).astype(np.int64)
    assert ix.quorum() == Q
    _, bc = ix.branches_info()
    bc = np.asarray(bc, dtype=np.int64)
    B = ix.num_branches()
    assert len(bc) == B and ff.gate(w, bc) and B % 4
    ev = ff.directed_events(branch, bc)
    hb, la, where = ff.directed_case(bc, seed=1)
    N = ff.N_DIRECTED
    hbe = np.zeros((len(d), B), dtype=np.uint32)
    lae = np.zeros((len(d), B), dtype=np.uint32)
    hbe[ev], lae[ev] = hb, la
    qa, qb = np.repeat(ev, N), np.tile(ev, N)
    m = ff.model(hbe, lae, bc, branch, w, qa, qb)
    predicted = ff.counters(m["rnd"])
    assert (m["early"] & (m["total"] >= Q)).any() and 0 < predicted[3] < predicted[1] < predicted[0] < N * N
    stride = write_rows(ix, ev, hb, la)
    assert stride > B                                   # pad columns: hb = 0x7FFFFFFF, la = 1
    got, fork_rounds, rounds = ask(ix, qa, qb)
    bad = np.flatnonzero(got != m["ans"])
    assert not len(bad), [(int(qa[i]), int(qb[i]), int(got[i]), int(m["rnd"][i])) for i in bad[:8]]
    assert fork_rounds == predicted
    assert rounds[0] == 0
    # the whole-row kernel on the same rows
    ix.set_option("fc_early_forks", 0)
    whole, fork_rounds, _ = ask(ix, qa, qb)
    assert fork_rounds == ZERO and whole.tobytes() == got.tobytes()
    ix.close()
