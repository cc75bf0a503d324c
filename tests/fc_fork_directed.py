"""Numpy model of the early exit in fork epochs (k_fc_fk_early, option
fc_early_forks) and the inputs of its tests.

The kernel reads both rows of a query in four rounds.  In columns, with
t0 = V // 4 and B branches:

  round 1  [0, 128), the originals [4 t0, V) of the straddling uint4 and every
           fork branch [V, B)
  round 2  [128, 256)     round 3  [256, 512)     round 4  [512, 4 t0)

The running count is the stake of the counting non-cheater originals read so
far plus the stake of every cheater one of whose branches has counted so far
(once per cheater); rest[r] is the stake of every validator whose original
column is unread after round r + 1.  A query stops after round r when its count
reached the quorum (true) or count + rest[r] cannot (false); HB(a)[branch(b)]
marked stops it after round 1 with the answer false.

  model          the reference's answers and the stopping round of given pairs
  gate           the host's conditions for taking the path at all
  oracle_planes  an oracle's HB / LA rows in plane form
  random_case    the DAGs, stakes and queries of tests/test_gpu_fc_early_forks.py
  directed_case  crafted rows on every quorum equality of every round

Shared by tests/test_fc_fork_directed_model.py (CPU: pins the model to the
oracle and checks what the inputs cover) and tests/test_gpu_fc_early_forks.py.
"""

import numpy as np

import fc_directed as fd

MARK = fd.MARK
MAX_INT32 = 0x7FFFFFFF
MAX_CHEATERS = 64
MIN_QUERIES = 1 << 14


def round_columns(V, B):
    """The plane columns of the four rounds."""
    c4 = V // 4 * 4
    r1 = np.concatenate([np.arange(0, min(128, c4)), np.arange(c4, B)])
    return [r1, np.arange(128, min(256, c4)), np.arange(256, min(512, c4)), np.arange(512, c4)]


def rests(w):
    """[rest after round 1, 2, 3, 4]: the stake of the validators whose original
    column is still unread."""
    w = np.asarray(w, dtype=np.uint64)
    c4 = len(w) // 4 * 4
    return [int(w[lo:c4].sum()) for lo in (128, 256, 512)] + [0]


def cheaters_of(bc, V):
    return np.flatnonzero(np.bincount(np.asarray(bc, dtype=np.int64), minlength=V) >= 2)


def gate(w, bc):
    """lx_fc_args' conditions on the epoch (the launch adds: >= 2^14 queries,
    a whole handle, the options): 1..64 cheaters, more than 512 original
    columns before the straddling uint4, a fork tail of <= 32 uint4, the
    validators of columns < 512 reach the quorum, rest[0] fits 32 bits."""
    w = np.asarray(w, dtype=np.uint64)
    V, B = len(w), len(bc)
    t0 = V // 4
    n_cheat = len(cheaters_of(bc, V))
    return bool(B > V and 1 <= n_cheat <= MAX_CHEATERS and t0 > 128 and (B + 3) // 4 - t0 <= 32 and
                int(w[:512].sum()) >= fd.quorum_of(w) and rests(w)[0] < 1 << 32)


def model(hb, la, bc, ev_branch, w, qa, qb, chunk=4096):
    """hb[E, B], la[E, B]: plane rows by event (bit 31 of hb: fork marker),
    bc[B] creator of each branch, ev_branch[E] branch of each event, w[V]
    stakes; qa, qb: event pairs.  Returns a dict: ans[n] the reference's
    answer (not early false and final count >= quorum), early[n], total[n]
    the final count, rnd[n] the round (1..4) the kernel stops at, cum[4, n]
    the running count after each round (of a query that gets there), rest[4]."""
    w = np.asarray(w, dtype=np.uint64)
    bc = np.asarray(bc, dtype=np.int64)
    V, B = len(w), len(bc)
    Q = fd.quorum_of(w)
    ch = cheaters_of(bc, V)
    is_ch = np.zeros(V, dtype=bool)
    is_ch[ch] = True
    k_of = np.full(V, -1, dtype=np.int64)
    k_of[ch] = np.arange(len(ch))
    rest = rests(w)
    n = len(qa)
    cum = np.zeros((4, n), dtype=np.int64)
    early = np.zeros(n, dtype=bool)
    wf = w.astype(np.float64)                                 # exact: every sum < 2^32
    for lo in range(0, n, chunk):
        a = np.asarray(qa[lo:lo + chunk], dtype=np.int64)
        b = np.asarray(qb[lo:lo + chunk], dtype=np.int64)
        h, l = hb[a][:, :B], la[b][:, :B]
        on = (l != 0) & (l <= h) & ((h & MARK) == 0)
        early[lo:lo + chunk] = (hb[a, np.asarray(ev_branch, dtype=np.int64)[b]] & MARK) != 0
        seen = np.zeros((len(a), len(ch)), dtype=bool)        # cheaters added so far
        acc = np.zeros(len(a), dtype=np.float64)
        for r, cols in enumerate(round_columns(V, B)):
            cr = bc[cols]
            plain = cols[~is_ch[cr] & (cols < V)]             # a non-cheater's fork branch does not exist
            acc = acc + on[:, plain].astype(np.float64) @ wf[plain]
            cc = cols[is_ch[cr]]
            if len(cc):
                hit = np.zeros((len(cc), len(ch)), dtype=np.float32)
                hit[np.arange(len(cc)), k_of[bc[cc]]] = 1
                seen |= (on[:, cc].astype(np.float32) @ hit) > 0
            cum[r, lo:lo + chunk] = (acc + seen.astype(np.float64) @ wf[ch]).astype(np.int64)
    rnd = np.full(n, 4, dtype=np.int64)
    still = np.ones(n, dtype=bool)
    for r in range(3):
        is_open = (cum[r] < Q) & (cum[r] + rest[r] >= Q)
        if r == 0:
            is_open &= ~early
        rnd[still & ~is_open] = r + 1
        still &= is_open
    total = cum[3]
    return {"ans": ~early & (total >= Q), "early": early, "total": total, "rnd": rnd, "cum": cum, "rest": rest,
            "quorum": Q}


def counters(rnd):
    """lx_fc_early_fork_rounds' four counts for queries stopping at rnd."""
    rnd = np.asarray(rnd)
    return (int((rnd >= 2).sum()), int((rnd >= 3).sum()), int(len(rnd)), int((rnd >= 4).sum()))


def oracle_planes(o, d, V):
    """The oracle's rows in plane form: hb[N, B] (a fork marker {0, MaxInt32}
    becomes bit 31 on every branch of that creator), la[N, B], the creator of
    each branch and the branch of each event."""
    N = len(d)
    B = o.num_branches()
    ev = np.arange(N, dtype=np.uint32)
    branch = np.array([o.branch(i) for i in range(N)], dtype=np.int64)
    bc = np.full(B, -1, dtype=np.int64)
    bc[branch] = d.creator
    assert np.all(bc >= 0) and np.array_equal(bc[:V], np.arange(V))
    hb = np.zeros((N, B), dtype=np.uint32)
    la = np.zeros((N, B), dtype=np.uint32)
    off, buf = o.rows(0, ev)
    forked = np.flatnonzero(np.bincount(bc, minlength=V) >= 2)
    fcols = np.flatnonzero(np.isin(bc, forked))
    for i in range(N):
        r = np.frombuffer(buf[int(off[i]):int(off[i + 1])].tobytes(), dtype=np.uint32).reshape(-1, 2)
        hb[i, :len(r)] = r[:, 0]
        fc = fcols[fcols < len(r)]
        marked = np.unique(bc[fc][(r[fc, 0] == 0) & (r[fc, 1] == MAX_INT32)])
        if len(marked):
            hb[i, np.isin(bc, marked)] |= MARK
    off, buf = o.rows(1, ev)
    for i in range(N):
        r = np.frombuffer(buf[int(off[i]):int(off[i + 1])].tobytes(), dtype=np.uint32)
        la[i, :len(r)] = r
    return hb, la, bc, branch


# ---------------------------------------------------------------- random fork DAGs
# name: (V, events per validator, cheaters, forks per cheater, cheaters heaviest?, seed, queries near / far)
RANDOM_CASES = {
    "516-1-heavy": (516, 24, 1, 3, True, 5, 40_000, 10_000),
    "516-40-light": (516, 20, 40, 2, False, 6, 40_000, 10_000),
    "600-3-light": (600, 20, 3, 3, False, 7, 60_000, 20_000),
    "1000-1-light": (1000, 16, 1, 3, False, 9, 150_000, 50_000),
    "1000-3-heavy": (1000, 16, 3, 3, True, 10, 60_000, 20_000),
    "1000-40-light": (1000, 16, 40, 2, False, 11, 20_000, 8_000),
}
WINDOW = 64


def zipf(V):
    return np.array([(1 << 20) // (i + 1) for i in range(V)], dtype=np.uint32)


def relabel(d, V, cheaters, heavy):
    """gen_dag's cheaters are creators 0..cheaters-1: the heaviest under Zipf
    stakes.  heavy = False renames creator c to V - 1 - c: they become the lightest."""
    if not heavy:
        d.creator = (V - 1 - d.creator.astype(np.int64)).astype(np.uint32)
    return d


def fork_dag(V, epv, cheaters, forks, heavy, seed):
    from lachesis_hip import tools
    return relabel(tools.gen_dag(V, epv, 10, cheaters=cheaters, forks=forks, seed=seed), V, cheaters, heavy)


def queries(d, near, far, seed, window=WINDOW):
    """Near pairs (b within `window` Lamport of a), far random pairs, and the
    far pairs in both orders."""
    from lachesis_hip import tools
    qa, qb = tools.fc_queries(d.lamport, near, window=window, seed=seed)
    rng = np.random.default_rng(seed)
    qa2 = rng.integers(0, len(d), far).astype(np.uint32)
    qb2 = rng.integers(0, len(d), far).astype(np.uint32)
    return np.concatenate([qa, qa2, qb2]), np.concatenate([qb, qb2, qa2])


def random_case(name):
    """(dag, stakes, qa, qb) of one case of the GPU test."""
    V, epv, ch, fk, heavy, seed, near, far = RANDOM_CASES[name]
    d = fork_dag(V, epv, ch, fk, heavy, seed)
    qa, qb = queries(d, near, far, seed)
    assert MIN_QUERIES <= len(qa) <= 250_000
    return d, zipf(V), qa, qb


# the gate: (V, events per validator, cheaters, forks, stakes, options, queries, fork-free path runs)
N14 = MIN_QUERIES
GATE_CASES = {
    "open": (600, 12, 3, 3, "zipf", {}, N14, False),
    "option-off": (600, 12, 3, 3, "zipf", {"fc_early_forks": 0}, N14, False),
    "fc_early-off": (600, 12, 3, 3, "zipf", {"fc_early": 0}, N14, False),
    "small-launch": (600, 12, 3, 3, "zipf", {}, N14 - 1, False),
    "V-512": (512, 12, 3, 3, "zipf", {}, N14, False),
    "V-516": (516, 12, 3, 3, "zipf", {}, N14, False),                  # open: the smallest V that takes the path
    "long-tail": (600, 12, 60, 4, "zipf", {}, N14, False),             # more than 128 fork branches
    "equal-stakes": (1000, 8, 3, 3, "equal", {}, N14, False),
    "fc_fk-off": (600, 12, 3, 3, "zipf", {"fc_fk": 0}, N14, False),
    "fork-free": (600, 12, 0, 0, "zipf", {}, N14, True),
}


GATE_OPEN = ("open", "V-516")


def gate_case(name):
    """(dag, stakes, qa, qb) of one case of the GPU test's gate test; the
    cheaters are the lightest validators."""
    V, epv, ch, fk, stakes, _, n, _ = GATE_CASES[name]
    d = fork_dag(V, epv, ch, fk, False, seed=31)
    w = zipf(V) if stakes == "zipf" else np.full(V, 3, dtype=np.uint32)
    qa, qb = queries(d, n - 4000, 2000, seed=32)
    assert len(qa) == n
    return d, w, qa, qb


# ---------------------------------------------------------------- directed rows
DIRECTED_V = 534          # t0 = 133: round 4 is columns [512, 532), 532 and 533 straddle into round 1
# the cheaters' creators: originals in round 2, round 3, round 4 and the straddling uint4
DIRECTED_CHEATERS = (140, 300, 530, 533)
DIRECTED_CHEATER_STAKES = (5, 7, 3, 2)
N_DIRECTED = 256


def directed_weights():
    """fd.edge_weights' design over this kernel's blocks: in every round's block
    the non-cheaters' stakes reach every integer up to their sum (round 1: 32
    of 1, 32 of 33, 64 of 1089 and the straddling 1; rounds 2, 3: four of 1,
    the rest 5; round 4 ones), round 1 alone exceeds the quorum."""
    V = DIRECTED_V
    w = np.ones(V, dtype=np.uint32)
    w[32:64] = 33
    w[64:128] = 33 * 33
    w[132:256] = 5
    w[260:512] = 5
    w[list(DIRECTED_CHEATERS)] = DIRECTED_CHEATER_STAKES
    return w


def directed_dag():
    """A small fork DAG whose four cheaters are the creators DIRECTED_CHEATERS."""
    from lachesis_hip import tools
    V = DIRECTED_V
    d = tools.gen_dag(V, 3, 10, cheaters=len(DIRECTED_CHEATERS), forks=2, seed=3)
    perm = np.arange(V, dtype=np.int64)
    for k, c in enumerate(DIRECTED_CHEATERS):
        perm[k], perm[c] = c, k
    d.creator = perm[d.creator.astype(np.int64)].astype(np.uint32)
    return d


def directed_events(branch, bc):
    """The N_DIRECTED events whose rows the directed test overwrites: the
    cheaters' events (up to 64, on original and fork branches: the b of an
    early false) last, other events first."""
    branch = np.asarray(branch, dtype=np.int64)
    tail = np.flatnonzero(np.isin(np.asarray(bc)[branch], DIRECTED_CHEATERS))[:64]
    assert (branch[tail] >= DIRECTED_V).any() and (branch[tail] < DIRECTED_V).any()
    head = np.setdiff1d(np.arange(len(branch)), tail)[:N_DIRECTED - len(tail)]
    return np.concatenate([head, tail]).astype(np.uint32)


def subset(w_eff, cols, target):
    """Columns of `cols` whose w_eff sum to exactly target (heaviest first; zero
    stakes are skipped); None when the greedy pick misses."""
    left = int(target)
    if left < 0:
        return None
    out = []
    for j in sorted((int(j) for j in cols), key=lambda j: (-int(w_eff[j]), j)):
        if w_eff[j] and int(w_eff[j]) <= left:
            out.append(j)
            left -= int(w_eff[j])
    return np.array(sorted(out), dtype=np.int64) if left == 0 else None


def directed_targets(W, R, Q):
    """{(round, cell): the four block sums} as fd.early_targets: the running
    count is open in every round before `round` and sits on the cell there.
    W[k]: what round k + 1's block can add, R[k]: rest after it."""
    out = {}
    for r in range(4):
        for cell in fd.EARLY_CELLS:
            if r == 3 and cell.startswith("r"):
                continue
            c = {"q": Q, "q-1": Q - 1, "r=q": Q - R[r], "r=q-1": Q - 1 - R[r]}[cell]
            cums = [0] * 4
            cums[r] = c
            ok = c >= 0
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
            t += [W[k] // 2 for k in range(r + 1, 4)]
            out[(r + 1, cell)] = tuple(t)
    return out


# the cheater rows: (name, base cell, cheater index, its columns that are set
# in the LA row: "o" original, "f" a fork branch).  The cheater's stake comes
# off the non-cheaters' sum of the round it first shows in, so the row sits on
# the base cell exactly when the kernel counts the cheater once, there.
CHEATER_ROWS = (
    ("fork-only", (1, "q"), 2, "f"),          # original in round 4, unset: counted through the branch in round 1
    ("fork-only-open", (2, "q"), 1, "f"),
    ("orig-only-r2", (2, "q"), 0, "o"),
    ("orig-only-r3", (3, "q"), 1, "o"),
    ("orig-only-r4", (4, "q"), 2, "o"),
    ("orig-only-straddle", (1, "q"), 3, "o"),
    ("both-r3", (3, "q-1"), 1, "of"),         # branch in round 1, original in round 3: once
    ("both-r4", (4, "q-1"), 2, "of"),
    ("both-r2-rest", (2, "r=q-1"), 0, "of"),
    ("both-straddle", (1, "q-1"), 3, "of"),
)


def directed_case(bc, seed=0):
    """Rows for the N_DIRECTED events of the directed test over the branch
    table bc of directed_dag(): (hb, la, where).  HB rows 0..7 count every set
    LA entry; rows 8..8+C-1 do too but mark cheater k (row 8 + k: bit 31 on
    all its branches); the rest are random edge-seq rows with random marks.
    LA rows: the targets of directed_targets (cheaters' columns unset), the
    CHEATER_ROWS, every column set, none; the rest random around the
    quorum's density.  where: {key: LA row}."""
    w = directed_weights()
    V, B = len(w), len(bc)
    bc = np.asarray(bc, dtype=np.int64)
    Q = fd.quorum_of(w)
    ch = np.array(DIRECTED_CHEATERS)
    assert np.array_equal(cheaters_of(bc, V), np.sort(ch))
    w_eff = w.copy()
    w_eff[ch] = 0
    blocks = [c[c < V] for c in round_columns(V, B)]
    W = [int(w_eff[c].astype(np.uint64).sum()) for c in blocks]
    R = rests(w)
    targets = directed_targets(W, R, Q)
    rng = np.random.default_rng(seed)
    n = N_DIRECTED
    hb, la = fd.random_rows(rng, n, B, 0.55 + 0.45 * rng.random(n))
    for i, v in enumerate(fd.FULL_HB):
        hb[i] = v
    n_full = len(fd.FULL_HB)
    for k, c in enumerate(ch):
        hb[n_full + k] = 0x7FFFFFFF
        hb[n_full + k, bc == c] |= MARK
    for i in range(n_full + len(ch), n):
        marked = ch[rng.random(len(ch)) < rng.choice([0.0, 0.1, 0.5])]
        hb[i, np.isin(bc, marked)] |= MARK

    def la_row(t, extra=()):
        row = np.zeros(B, dtype=np.uint32)
        for cols, tk in zip(blocks, t):
            s = subset(w_eff, cols, tk)
            assert s is not None, tk
            row[s] = 1
        row[list(extra)] = 1
        return row

    where = {}
    k = 0
    for key, t in sorted(targets.items()):
        la[k] = la_row(t)
        where[key] = k
        k += 1
    first_round = {c: next(r for r, cols in enumerate(round_columns(V, B)) if c in cols) for c in range(B)}
    for name, cell, ci, which in CHEATER_ROWS:
        c = int(ch[ci])
        cols = []
        if "o" in which:
            cols.append(c)
        if "f" in which:
            cols.append(int(np.flatnonzero(bc == c)[-1]))
        t = list(targets[cell])
        shows = min(first_round[x] for x in cols)
        assert shows < cell[0]
        t[shows] -= int(w[c])
        la[k] = la_row(t, cols)
        where[name] = k
        k += 1
    la[k], la[k + 1] = 1, 0
    where["all"], where["none"] = k, k + 1
    # the last rows belong to cheaters' events (directed_events): an early
    # false over a count that reaches the quorum, and over none
    la[n - 1], la[n - 2] = 1, 0
    return hb, la, where
