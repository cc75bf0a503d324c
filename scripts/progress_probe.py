#!/usr/bin/env python3
"""Latency of lx_abft_build_progress against lx_abft_build_frames on the same
handle and the same candidates.

The shape and the candidates of scripts/build_probe.py (BASELINE configs[4]:
V = 1000 Zipf stakes, 50 events per validator, 10 parents, the whole epoch
processed first; one candidate per validator -- its last event plus the last
events of the next nine validators).  Per iteration, one after the other on
one handle:

* ``frames_n1`` / ``frames_n1000``      : lx_abft_build_frames, the yardstick;
* ``progress_n1`` / ``progress_n1000``  : lx_abft_build_progress without pairs;
* ``pairs_n1`` / ``pairs_n1000``        : with LX_PROGRESS_PAIRS, the read of
  the pair list through lx_abft_last_progress_pairs timed apart
  (``read_n1`` / ``read_n1000``).

Host clocks around calls that end in a device synchronise, ctypes overhead
included.  Prints one JSON line: p50 / p10 / p90 in microseconds, the
differences of the medians against the yardstick, the GPU work
lx_abft_build_last_stats reports; checks that the frames agree and that
stake < quorum at every Build frame.  Needs the GPU.
"""

import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "lachesis-base_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

u8p = ctypes.POINTER(ctypes.c_uint8)
u32p = ctypes.POINTER(ctypes.c_uint32)
u64p = ctypes.POINTER(ctypes.c_uint64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--validators", type=int, default=1000)
    ap.add_argument("--events-per-validator", type=int, default=50)
    ap.add_argument("--parents", type=int, default=10)
    args = ap.parse_args()

    import lachesis_hip as lx

    V, epv, P = args.validators, args.events_per_validator, args.parents
    weights = [(1 << 20) // (i + 1) for i in range(V)]
    quorum = sum(weights) * 2 // 3 + 1
    dag = lx.tools.gen_dag(V, epv, P, 0, 0, seed=1)
    N = len(dag)
    lch = lx.abft.DenseLachesis(weights, event_capacity=N + 8, apply_events=False, block_log=True)
    rc, consumed, frames = lch.process_batch(dag.creator, dag.seq, dag.poff, dag.par)
    assert rc == 0 and consumed == N

    last = np.zeros(V, dtype=np.int64)
    last[dag.creator] = np.arange(N)                         # Add order: the last write is the last event
    cr = np.arange(V, dtype=np.uint32)
    sq = (dag.seq[last] + 1).astype(np.uint32)
    par = np.stack([last[(cr + k) % V] for k in range(min(P, V))], axis=1).astype(np.uint32)
    np_ = par.shape[1]
    off = (np.arange(V + 1, dtype=np.uint64) * np_)
    flat = np.ascontiguousarray(par.reshape(-1))
    L, h = lch.L, lch.h
    P32 = lambda a: a.ctypes.data_as(u32p)
    P64 = lambda a: a.ctypes.data_as(u64p)

    def outs(n):
        return [np.zeros(n, dtype=np.uint32) for _ in range(4)] + [np.zeros(n, dtype=np.uint64)]
    o_all, o1 = outs(V), outs(1)
    fr_all, fr1 = np.zeros(V, dtype=np.uint32), np.zeros(1, dtype=np.uint32)
    root_all, root1 = np.zeros(V, dtype=np.uint8), np.zeros(1, dtype=np.uint8)
    off1 = np.array([0, np_], dtype=np.uint64)
    err = ctypes.c_uint32()
    total = ctypes.c_uint64()
    cap = V * 4096
    pr_off, pr_root, pr_stake = np.zeros(V + 1, dtype=np.uint64), np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.uint32)
    names = ("frames_n1", "progress_n1", "pairs_n1", "read_n1", "frames_n%d" % V, "progress_n%d" % V,
             "pairs_n%d" % V, "read_n%d" % V)
    t = {k: [] for k in names}
    stats, n_pairs = {}, {}

    def timed(name, fn, keep):
        t0 = time.perf_counter_ns()
        rc = fn()
        t1 = time.perf_counter_ns()
        assert rc == 0, L.lx_abft_last_error(h)
        if keep:
            t[name].append(t1 - t0)

    for it in range(args.warmup + args.iters):
        i = (it * 37) % V
        keep = it >= args.warmup
        pi = np.ascontiguousarray(par[i])
        c1, s1 = cr[i:i + 1], sq[i:i + 1]

        def progress(n, c, s, o, p, out, flags):
            return L.lx_abft_build_progress(h, n, P32(c), P32(s), P64(o), P32(p), None, flags, P32(out[0]), P32(out[1]),
                                            P32(out[2]), P32(out[3]), P64(out[4]), ctypes.byref(err))

        def read():
            return L.lx_abft_last_progress_pairs(h, P64(pr_off), P32(pr_root), P32(pr_stake), cap, ctypes.byref(total))
        timed(names[0], lambda: L.lx_abft_build_frames(h, 1, P32(c1), P32(s1), P64(off1), P32(pi), P32(fr1),
                                                       root1.ctypes.data_as(u8p), ctypes.byref(err)), keep)
        timed(names[1], lambda: progress(1, c1, s1, off1, pi, o1, 0), keep)
        if it == args.warmup:
            stats["progress_n1"] = lch.build_stats()
        timed(names[2], lambda: progress(1, c1, s1, off1, pi, o1, 1), keep)
        timed(names[3], read, keep)
        n_pairs["n1"] = total.value
        assert int(o1[0][0]) == int(fr1[0]) and int(o1[3][0]) < quorum and total.value == int(o1[1][0])
        timed(names[4], lambda: L.lx_abft_build_frames(h, V, P32(cr), P32(sq), P64(off), P32(flat), P32(fr_all),
                                                       root_all.ctypes.data_as(u8p), ctypes.byref(err)), keep)
        if it == args.warmup:
            stats["frames_n%d" % V] = lch.build_stats()
        timed(names[5], lambda: progress(V, cr, sq, off, flat, o_all, 0), keep)
        if it == args.warmup:
            stats["progress_n%d" % V] = lch.build_stats()
        timed(names[6], lambda: progress(V, cr, sq, off, flat, o_all, 1), keep)
        timed(names[7], read, keep)
        n_pairs["n%d" % V] = total.value
        assert np.array_equal(o_all[0], fr_all) and int(o_all[3].max()) < quorum
        assert total.value == int(o_all[1].sum()) <= cap and int(o_all[0][i]) == int(fr1[0])

    def us(a):
        a = np.array(a) / 1e3
        return {"p50": round(float(np.percentile(a, 50)), 2), "p10": round(float(np.percentile(a, 10)), 2),
                "p90": round(float(np.percentile(a, 90)), 2)}
    res = {"shape": [V, epv, P], "events": N, "iters": args.iters, "max_frame": int(frames.max()), "quorum": quorum,
           "pairs": n_pairs, "candidates_with_stake": int((o_all[3] > 0).sum()),
           "caused_pairs": int(o_all[2].sum())}
    for k in names:
        res[k + "_us"] = us(t[k])
    med = lambda k: float(np.percentile(t[k], 50)) / 1e3
    for n in ("n1", "n%d" % V):
        res["progress_minus_frames_%s_us_p50" % n] = round(med("progress_" + n) - med("frames_" + n), 2)
        res["pairs_minus_frames_%s_us_p50" % n] = round(med("pairs_" + n) - med("frames_" + n), 2)
    res["gpu_work"] = stats
    print(json.dumps(res))
    lch.close()


if __name__ == "__main__":
    main()
