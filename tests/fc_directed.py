"""Reference and row constructors for the directed ForklessCause tests.

ForklessCause is a stake-weighted count compared with a quorum
(vecfc/forkless_cause.go:40-82, inter/pos/stake.go:47-55).  The helpers here
work on plane-form rows (lx_internal.h: hb[e][b] the raw HighestBefore seq with
bit 31 = fork marker of creator(b), la[e][b] the LowestAfter seq, 0 = none):

  ref_sums       the exact sum of every (a, b) pair and its early false, numpy
  early_model    the round at which k_fc_early must stop for every pair
  edge_weights   stakes whose block subsets reach every integer, so a row can
                 be placed exactly on a quorum equality in any round
  subset_with_weight  the columns of such a subset

Shared by tests/test_fc_directed_model.py (CPU: pins the reference to the
oracle) and tests/test_gpu_fc_directed.py (the kernels on crafted rows).
"""

import numpy as np

MARK = 0x80000000
# seq values at which an entry's handling may change: none / first, the 16-bit
# boundary, the largest seq
EDGE_SEQS = (0, 1, 2, 3, 0xFFFE, 0xFFFF, 0x10000, 0x10001, 0x7FFFFFFE, 0x7FFFFFFF)


def quorum_of(w):
    return int(np.asarray(w, dtype=np.uint64).sum()) * 2 // 3 + 1


def counting(hb_row, la):
    """Columns that count for one HighestBefore row against LowestAfter rows
    la[Nb, B]: la != 0, la <= hb, and hb not marked."""
    return (la != 0) & (la <= hb_row[None, :]) & ((hb_row & MARK) == 0)[None, :]


def ref_sums(hb, la, w, branch_creator=None, b_branch=None):
    """Exact ForklessCause sums of all pairs: hb[Na, B] rows of the a events,
    la[Nb, B] rows of the b events, w[V] stakes.  Fork-free (branch_creator
    None, B == V): sum_j w[j] * (la[j] != 0 and la[j] <= hb[j]).  With forks:
    branch_creator[B] maps columns to creators, a creator counts once if any of
    its branches counts, a marked hb never counts, and b_branch[Nb] (the branch
    of each b) gives the early false: hb(a)[branch(b)] marked.  Returns
    (sum[Na, Nb] uint64, early_false[Na, Nb] bool); the answer is
    not early_false and sum >= quorum."""
    hb = np.asarray(hb, dtype=np.uint32)
    la = np.asarray(la, dtype=np.uint32)
    w = np.asarray(w, dtype=np.uint64)
    Na, Nb = len(hb), len(la)
    sums = np.zeros((Na, Nb), dtype=np.uint64)
    early = np.zeros((Na, Nb), dtype=bool)
    if branch_creator is None:
        assert hb.shape[1] == la.shape[1] == len(w)
        for i in range(Na):
            sums[i] = counting(hb[i], la).astype(np.uint64) @ w
        return sums, early
    bc = np.asarray(branch_creator, dtype=np.int64)
    assert hb.shape[1] == la.shape[1] == len(bc)
    order = np.argsort(bc, kind="stable")
    starts = np.searchsorted(bc[order], np.arange(len(w)))     # every creator owns its original branch
    assert np.array_equal(bc[order][starts], np.arange(len(w)))
    for i in range(Na):
        c = counting(hb[i], la)[:, order].astype(np.uint32)
        by_creator = np.add.reduceat(c, starts, axis=1) > 0
        sums[i] = by_creator.astype(np.uint64) @ w
    if b_branch is not None:
        early = (hb[:, np.asarray(b_branch, dtype=np.int64)] & MARK) != 0
    return sums, early


def early_blocks(V, L):
    """Column blocks of k_fc_early's four rounds with L lanes per query."""
    return [(0, min(4 * L, V)), (min(4 * L, V), min(8 * L, V)), (min(8 * L, V), min(16 * L, V)), (min(16 * L, V), V)]


def early_model(hb, la, w, quorum, L):
    """The round (1, 2, 3, or 4 = the rest of the rows) at which k_fc_early
    stops for every pair of fork-free rows: it reads the blocks [0, 4L),
    [4L, 8L), [8L, 16L), [16L, V) in turn and reads on only while the count so
    far leaves the quorum open, sum < quorum <= sum + (stake of the unread
    columns) -- the bounds lx_fc_args computes from the actual stakes.
    Returns (round[Na, Nb], cum[4, Na, Nb], rest[4], gate): cum[r] the count
    after round r + 1 of a query that got there, rest[r] the stake unread
    after it, gate whether the first 16L columns reach the quorum alone (the
    host's condition for taking the early path at all)."""
    w = np.asarray(w, dtype=np.uint64)
    V = len(w)
    blocks = early_blocks(V, L)
    cum = np.zeros((4, len(hb), len(la)), dtype=np.uint64)
    rest = []
    acc = np.zeros((len(hb), len(la)), dtype=np.uint64)
    for r, (lo, hi) in enumerate(blocks):
        s, _ = ref_sums(hb[:, lo:hi], la[:, lo:hi], w[lo:hi])
        acc = acc + s
        cum[r] = acc
        rest.append(int(w[hi:].sum()))
    rnd = np.full(acc.shape, 4, dtype=np.int64)
    still = np.ones(acc.shape, dtype=bool)
    for r in range(3):
        c = cum[r].astype(np.int64)
        is_open = (c < quorum) & (c + rest[r] >= quorum)
        rnd[still & ~is_open] = r + 1
        still &= is_open
    gate = int(w[:blocks[2][1]].sum()) >= quorum
    return rnd, cum, rest, gate


def edge_weights(V, L):
    """Stakes for the early-exit tests: inside every round's block each integer
    in [0, W_block] is a subset sum, by mixed radix.  Block 0 (n = 4L columns,
    a = n / 4): a columns of 1, a of a + 1, the rest of (a + 1)^2; blocks 1
    and 2: 4 columns of 1 and the rest of 5; the last block all ones.  Block
    0 alone then exceeds the quorum, and every later block is heavy enough to
    carry the quorum equalities of its round.

    The stakes are NOT in descending order: lx_reset does not require it (only
    pos.Validators sorts), and the early exit's bounds are sums of the actual
    stakes of the unread columns, whatever their order."""
    w = np.ones(V, dtype=np.uint32)
    blocks = early_blocks(V, L)
    lo, hi = blocks[0]
    a = (hi - lo) // 4
    w[lo + a:lo + 2 * a] = a + 1
    w[lo + 2 * a:hi] = (a + 1) ** 2
    for lo, hi in blocks[1:3]:
        w[lo + 4:hi] = 5
    assert int(w.astype(np.uint64).sum()) < 1 << 31
    return w


def subset_with_weight(w, lo, hi, target):
    """Columns of [lo, hi) whose stakes sum to exactly `target`, picked greedily
    from the heaviest down (exact for edge_weights' blocks, all-ones and
    powers of two); None when the greedy pick misses."""
    w = np.asarray(w, dtype=np.uint64)
    left = int(target)
    if left < 0:
        return None
    cols = []
    for j in sorted(range(lo, hi), key=lambda j: (-int(w[j]), j)):
        if int(w[j]) <= left and w[j]:
            cols.append(j)
            left -= int(w[j])
    return np.array(sorted(cols), dtype=np.int64) if left == 0 else None


# ---------------------------------------------------------------- early-exit targets
# One target per (stopping round, cell): a tuple of the four block sums whose
# running count is open in every round before `round` and sits on the cell in
# `round`.  Cells: the count equals the quorum ("q"), the quorum - 1 ("q-1"),
# or count + unread stake equals the quorum ("r=q") or the quorum - 1 ("r=q-1").
EARLY_CELLS = ("q", "q-1", "r=q", "r=q-1")


def early_targets(w, L):
    """{(round, cell): (t0, t1, t2, t3)} for every cell that applies (the last
    round has nothing unread: only "q" and "q-1")."""
    w = np.asarray(w, dtype=np.uint64)
    V = len(w)
    Q = quorum_of(w)
    blocks = early_blocks(V, L)
    W = [int(w[lo:hi].sum()) for lo, hi in blocks]
    R = [sum(W[r + 1:]) for r in range(4)]            # unread after round r + 1
    out = {}
    for r in range(4):
        for cell in EARLY_CELLS:
            if r == 3 and cell.startswith("r"):
                continue
            c = {"q": Q, "q-1": Q - 1, "r=q": Q - R[r], "r=q-1": Q - 1 - R[r]}[cell]
            cums = [0] * 4
            cums[r] = c
            ok = 0 <= c
            # back-fill: the count after round k must leave the quorum open,
            # Q - R[k] <= c_k <= Q - 1, and differ from c_{k+1} by a block sum
            for k in range(r - 1, -1, -1):
                lo_ = max(Q - R[k], cums[k + 1] - W[k + 1], 0)
                hi_ = min(Q - 1, cums[k + 1])
                if lo_ > hi_:
                    ok = False
                    break
                cums[k] = (lo_ + hi_) // 2
            if not ok or cums[0] > W[0]:
                continue
            t = [cums[0]] + [cums[k] - cums[k - 1] for k in range(1, r + 1)]
            # blocks after the stopping round: half full, they must not matter
            t += [W[k] // 2 for k in range(r + 1, 4)]
            out[(r + 1, cell)] = tuple(t)
    return out


def la_row_for(w, L, t):
    """A LowestAfter row (entries 1 / 0) whose four block sums are t."""
    V = len(w)
    row = np.zeros(V, dtype=np.uint32)
    for (lo, hi), tk in zip(early_blocks(V, L), t):
        cols = subset_with_weight(w, lo, hi, tk)
        assert cols is not None, (lo, hi, tk)
        row[cols] = 1
    return row


FULL_HB = (1, 0x7FFFFFFF, 0xFFFF, 0x10000, 2, 0x7FFFFFFE, 0xFFFE, 0x10001)


def random_rows(rng, n, cols, p_count):
    """n HighestBefore and n LowestAfter rows of edge seqs; p_count[i] steers
    how many columns of row i can count (hb large / la small and non-zero)."""
    e = np.array(EDGE_SEQS, dtype=np.uint32)
    hb = e[rng.integers(0, len(e), (n, cols))]
    la = e[rng.integers(0, len(e), (n, cols))]
    big = rng.random((n, cols)) < np.asarray(p_count)[:, None]
    hb = np.where(big, np.maximum(hb, np.uint32(0x10001)), hb).astype(np.uint32)
    small = rng.random((n, cols)) < np.asarray(p_count)[:, None]
    la = np.where(small, np.clip(la, 1, 0x10001), la).astype(np.uint32)
    return hb, la


def early_rows(w, L, n=256, seed=0):
    """n HighestBefore and n LowestAfter rows (fork-free, V columns) for the
    early-exit test.  HB rows 0..7 count every set LA entry (one constant edge
    seq each, the first equal to the LA entries: la == hb); the first LA rows
    are early_targets' rows, so each (full HB row, target row) pair sits on
    its cell; the rest are random edge-seq rows around the quorum's density,
    whose pairs with the target rows give counts just below the cells.
    Returns (hb, la, {cell key: LA row index})."""
    V = len(w)
    rng = np.random.default_rng(seed)
    p = 0.55 + 0.45 * rng.random(n)
    hb, la = random_rows(rng, n, V, p)
    for i, v in enumerate(FULL_HB):
        hb[i] = v
    where = {}
    for k, (key, t) in enumerate(sorted(early_targets(w, L).items())):
        la[k] = la_row_for(w, L, t)
        where[key] = k
    # every column set / none
    la[n - 1] = 1
    la[n - 2] = 0
    return hb, la, where


def early_cells(rnd, cum, rest, quorum):
    """{(round, cell): number of queries that reached `round` and sit on the
    cell there}, from early_model's outputs alone."""
    out = {}
    for r in range(4):
        reached = rnd >= r + 1
        c = cum[r].astype(np.int64)
        for cell in EARLY_CELLS:
            if r == 3 and cell.startswith("r"):
                continue
            v = {"q": quorum, "q-1": quorum - 1, "r=q": quorum - rest[r], "r=q-1": quorum - 1 - rest[r]}[cell]
            out[(r + 1, cell)] = int((reached & (c == v)).sum())
    return out


# ---------------------------------------------------------------- whole-row tests
# columns at which a lane, a round or a loop of the kernels changes: a uint4's
# first / last word, the early rounds' block bounds for 32 and 16 lanes, and
# both sides of column 1024 (rows longer than 4 uint4 per lane of 64)
SINGLE_COLS = (0, 3, 4, 63, 64, 127, 128, 255, 256, 511, 512, 1023, 1024, 1027)


def whole_row_weights(V, seed=0):
    """{name: stakes} of the whole-row test: all ones; 2^j (V <= 30: the sum
    names the columns that counted); random stakes whose total is exactly
    lx_reset's limit 0x7FFFFFFF; one validator holding all of that limit but
    one unit for each of the others."""
    rng = np.random.default_rng(seed)
    T = 0x7FFFFFFF
    out = {"ones": np.ones(V, dtype=np.uint32)}
    if V <= 30:
        out["pow2"] = (np.uint32(1) << np.arange(V, dtype=np.uint32)).astype(np.uint32)
    r = rng.random(V) ** 4                                   # skewed: a few heavy, many light
    w = np.floor(r / r.sum() * (T - V)).astype(np.uint64) + 1
    w[int(rng.integers(V))] += T - int(w.sum())
    assert int(w.sum()) == T and w.min() >= 1
    out["random_max_total"] = w.astype(np.uint32)
    big = np.ones(V, dtype=np.uint32)
    big[0] = T - (V - 1)
    out["one_heavy"] = big
    return out


def whole_rows(w, n=256, seed=0):
    """n HighestBefore and n LowestAfter rows (fork-free, V columns) for the
    whole-row test: HB rows 0..7 count every set LA entry; LA rows: one per
    SINGLE_COLS column (and V - 1) with only that column set, subsets of
    weight quorum - 1 / quorum / quorum + 1 where the stakes allow them
    exactly, every column at 1, none, every column at 2 (= hb + 1 for HB row
    0, = hb for row 4); the rest random edge seqs of every density.  Returns
    (hb, la, quorum LA rows {delta: row})."""
    V = len(w)
    rng = np.random.default_rng(seed)
    hb, la = random_rows(rng, n, V, rng.random(n))
    for i, v in enumerate(FULL_HB):
        hb[i] = v
    k = 0
    for c in sorted(set(SINGLE_COLS) | {V - 1}):
        if c < V:
            la[k] = 0
            la[k, c] = 1
            k += 1
    Q = quorum_of(w)
    qrows = {}
    for delta in (-1, 0, 1):
        cols = subset_with_weight(w, 0, V, Q + delta)
        if cols is not None:
            la[k] = 0
            la[k, cols] = 1
            qrows[delta] = k
            k += 1
    la[k], la[k + 1], la[k + 2] = 1, 0, 2
    return hb, la, qrows


def pad_rows(rows, stride, value):
    """rows[n, cols] widened to the plane's stride; the pad columns hold
    `value`: entries that would count if a kernel read them with a stake."""
    out = np.full((len(rows), stride), value, dtype=np.uint32)
    out[:, :rows.shape[1]] = rows
    return out


def mixed_radix_weights(V):
    """Stakes over a whole row of which every integer in [0, total] is a subset
    sum (V >= 8): with a = V / 4, columns j % 4 == 0 hold 1, j % 4 == 1 hold
    a + 1, the others (a + 1)^2 -- at least a of each of the two light kinds.
    Neighbouring validators differ in stake, so a miscounted creator shows."""
    a = V // 4
    j = np.arange(V)
    w = np.where(j % 4 == 0, 1, np.where(j % 4 == 1, a + 1, (a + 1) ** 2)).astype(np.uint32)
    assert int(w.astype(np.uint64).sum()) < 1 << 31
    return w


def fork_rows(branch_creator, w, n=256, seed=0):
    """n HighestBefore and n LowestAfter rows over the B columns of a fork
    DAG's branch table.  HB rows 0..7 count every set LA entry; every other
    row marks a random set of the cheaters (creators with more than one
    branch): bit 31 on ALL of the creator's branch columns, over a raw seq
    that would count without it.  Returns (hb, la, quorum LA rows {delta:
    row}): creators of weight quorum + delta, each counting through its LAST
    branch only (a fork branch, for a cheater)."""
    bc = np.asarray(branch_creator, dtype=np.int64)
    B, V = len(bc), len(w)
    rng = np.random.default_rng(seed)
    hb, la = random_rows(rng, n, B, rng.random(n))
    cheaters = np.flatnonzero(np.bincount(bc, minlength=V) >= 2)
    for i, v in enumerate(FULL_HB):
        hb[i] = v
    for i in range(len(FULL_HB), n):
        marked = cheaters[rng.random(len(cheaters)) < rng.choice([0.0, 0.1, 0.5])]
        hb[i, np.isin(bc, marked)] |= MARK
    # rows whose only counting column is a fork branch (the per-creator
    # dedupe must add the creator's stake although its original is silent),
    # and the original plus all of its fork branches (once, not per branch)
    k = 0
    for c in cheaters[:4]:
        cols = np.flatnonzero(bc == c)
        la[k] = 0
        la[k, cols[-1]] = 1
        la[k + 1] = 0
        la[k + 1, cols] = 1
        k += 2
    la[k], la[k + 1] = 1, 0
    k += 2
    last_branch = np.zeros(V, dtype=np.int64)
    last_branch[bc] = np.arange(B)                            # ascending: the last branch of each creator wins
    Q = quorum_of(w)
    qrows = {}
    for delta in (-1, 0, 1):
        creators = subset_with_weight(w, 0, V, Q + delta)
        if creators is not None:
            la[k] = 0
            la[k, last_branch[creators]] = 1
            qrows[delta] = k
            k += 1
    return hb, la, qrows
