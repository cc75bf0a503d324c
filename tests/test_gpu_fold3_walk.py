"""The three-input fold (F3: v_pk_maximum3_f16 in the 8- / 12-column packed
walks, chosen per launch while the epoch's max_seq <= 0x7BFF; option fold3 = 0
forces the integer fold) on whole walks, at the seq where it switches off.

Inputs are the two-speed DAGs of tests/seq16_dags.py (one creator reaches seq
0x7C00 in ~70k events): V = 13 (two 12-column slices, the second with one
valid column) and V = 25, epochs whose max_seq is 0x7BFF and 0x7C00 (the
0x7BFF epoch is the 0x7C00 one without its last level), each as one batch and
as two batches -- the 0x7BFF epoch cut at level 0x7BC0, so batch 2 has parents
from batch 1 and ends with the handle at exactly 0x7BFF; the 0x7C00 epoch cut
at level 0x7BFF, so the handle sits at 0x7BFF and then crosses -- with cpw 8
and 12 and segments 0 and 3.  Every HighestBefore and LowestAfter row must
equal the C oracle's, and the rows of the fold3 = 0 handle must equal the
fold3 = 1 handle's byte for byte.

test_many_parents: a short epoch in which events take the latest event of
every other validator as parents (25 > 12 inline parents: the extra-parent
path folds integer maxima into the lane's packed unit), whole and cut in two.

test_segment_stats_unchanged: on default options fold3 changes nothing that
lx_last_segment_stats reports (segments and their first events, partial
events, one_launch; the slice width is not reported, the first events and
one_launch follow from it): the option switches only the fold.

Measured on an MI355X: the module in 4 s; test_walks_at_the_fold3_boundary
0.16-0.41 s per case (the first 2.0 s: it builds the DAGs and the oracle's
rows), test_many_parents 0.01-0.03 s, test_segment_stats_unchanged 0.03 s.
"""

import numpy as np
import pytest

from oracle import corc
import seq16_dags as sd
from seq16_dags import level_end

pytestmark = pytest.mark.gpu

F, EVERY, SEED = 2, 64, 5
L_LAST, L_FIRST = 0x7BFF, 0x7C00     # the last epoch length the F3 fold takes, the first it does not
CUT_BEFORE = 0x7BC0
WEIGHTS = {V: [3, 3] + [1] * (V - 2) for V in (13, 25)}


@pytest.fixture(scope="module")
def lx():
    import lachesis_hip
    return lachesis_hip


def many_parents(d):
    """d with the parents of fast validator 0's events at levels = 2 mod every
    replaced by its self-parent and the latest event of every other validator."""
    V = d.n_nodes
    last, lam, poff, par = [-1] * V, [], [0], []
    for e in range(len(d)):
        c = int(d.creator[e])
        ps = [int(p) for p in d.par[int(d.poff[e]):int(d.poff[e + 1])]]
        if c == 0 and d.level[e] % d.every == 2 and last[0] >= 0:
            ps = [last[0]] + [last[v] for v in range(1, V) if last[v] >= 0]
        lam.append(1 + max((lam[p] for p in ps), default=0))
        par.extend(ps)
        poff.append(len(par))
        last[c] = e
    w = sd.Dag(d.creator, d.seq, np.array(lam, dtype=np.uint32), np.array(poff, dtype=np.uint64),
               np.array(par, dtype=np.uint32), V)
    w.level, w.level_ends = d.level, d.level_ends
    return w


class World:
    """DAGs, oracles and the oracles' rows, each built once per module and
    never modified afterwards."""

    def __init__(self):
        self._dag, self._rows = {}, {}

    def dag(self, V, wide=False):
        if (V, wide) not in self._dag:
            self._dag[V, wide] = (many_parents(sd.two_speed(V, F, 0x400, EVERY, SEED)) if wide
                                  else sd.two_speed(V, F, L_FIRST, EVERY, SEED))
        return self._dag[V, wide]

    def rows(self, V, n, wide=False):
        """The oracle's HighestBefore and LowestAfter rows of events 0..n-1."""
        if (V, n, wide) not in self._rows:
            d = self.dag(V, wide)
            o = corc.OracleIndex(WEIGHTS[V])
            assert o.add_batch(d.creator[:n], d.seq[:n], d.poff[:n + 1], d.par) == -1
            ev = np.arange(n, dtype=np.uint32)
            self._rows[V, n, wide] = [o.rows(mode, ev) for mode in (0, 1)]
        return self._rows[V, n, wide]


@pytest.fixture(scope="module")
def world():
    return World()


def walk(lx, d, V, cuts, **options):
    """The rows of events 0..cuts[-1]-1 of a handle fed the batches between the cuts."""
    n = cuts[-1]
    ix = lx.Index(event_capacity=n, options=dict(small_max=0, dbl=0, **options))
    ix.reset(WEIGHTS[V])
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        ix.add_batch(d.creator[lo:hi], d.seq[lo:hi], d.poff[lo:hi + 1], d.par)
    assert ix.num_events() == n and ix.num_branches() == V
    ev = np.arange(n, dtype=np.uint32)
    got = [ix.rows_np(mode, ev) for mode in (0, 1)]
    ix.close()
    return got


def check(lx, world, V, cuts, wide=False, **options):
    d = world.dag(V, wide)
    want = world.rows(V, cuts[-1], wide)
    got = {f3: walk(lx, d, V, cuts, fold3=f3, **options) for f3 in (1, 0)}
    for mode in (0, 1):
        for k in (0, 1):      # offsets, bytes
            assert np.array_equal(got[1][mode][k], want[mode][k]), ("fold3=1 against the oracle", mode, cuts)
            assert np.array_equal(got[0][mode][k], got[1][mode][k]), ("fold3=0 against fold3=1", mode, cuts)


@pytest.mark.parametrize("segments", [0, 3])
@pytest.mark.parametrize("cpw", [8, 12])
@pytest.mark.parametrize("V", [13, 25])
def test_walks_at_the_fold3_boundary(lx, world, V, cpw, segments):
    d = world.dag(V)
    n_cut, n_last, n_first = (level_end(d, L) for L in (CUT_BEFORE, L_LAST, L_FIRST))
    assert int(d.seq[:n_last].max()) == L_LAST and int(d.seq[:n_first].max()) == L_FIRST
    # batch 2 of the cut 0x7BFF epoch takes parents from batch 1
    assert int(d.par[int(d.poff[n_cut]):int(d.poff[n_last])].min()) < n_cut
    for cuts in ([0, n_last], [0, n_cut, n_last], [0, n_first], [0, n_last, n_first]):
        check(lx, world, V, cuts, cpw=cpw, segments=segments)


@pytest.mark.parametrize("segments", [0, 3])
@pytest.mark.parametrize("cpw", [8, 12])
def test_many_parents(lx, world, cpw, segments):
    V = 25
    d = world.dag(V, wide=True)
    n = len(d)
    assert int(np.diff(d.poff.astype(np.int64)).max()) == V > 12 and n // 2 >= 64 * 3
    for cuts in ([0, n], [0, n // 2, n]):
        check(lx, world, V, cuts, wide=True, cpw=cpw, segments=segments)


def test_segment_stats_unchanged(lx, world):
    V = 25
    d = world.dag(V)
    n = level_end(d, L_LAST)
    st = {}
    for f3 in (1, 0):
        ix = lx.Index(event_capacity=n, options={"fold3": f3})
        ix.reset(WEIGHTS[V])
        ix.add_batch(d.creator[:n], d.seq[:n], d.poff[:n + 1], d.par)
        ix.sync()
        s = ix.segment_stats()
        st[f3] = {k: s[k] for k in ("segments", "first_event", "partial", "one_launch")}
        ix.close()
    assert st[1]["segments"] >= 2, st[1]       # the default handle splits this batch on its own
    assert st[0] == st[1]
