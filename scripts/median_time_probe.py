#!/usr/bin/env python3
"""Latency of lx_mt_median_time against what a caller did without it.

On the V = 1000 Zipf shape (tdag.rand_fork_dag(1000, 3, 10, seed=5), the
shape of tests/test_gpu_median_time.py) for n = 1 and n = 256 events:

* ``mt``   : one lx_mt_median_time call (the medians come back, 8 n bytes);
* ``host`` : lx_get_merged_highest_before_batch (8 V bytes per event come
  back), then the caller's own (validator, seq) -> time table and a weighted
  median per event in numpy.

Both are host clocks around calls that end in a device synchronise, ctypes
call overhead included on both sides; the two alternate inside one loop.
Prints one JSON line (p50 / p10 / p90 in microseconds) and checks that both
ways give the same medians.  Needs the GPU.
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
    ap.add_argument("--default-time", type=int, default=1010)
    args = ap.parse_args()

    import lachesis_hip as lx
    from oracle import pos, tdag

    V = 1000
    nodes, events = tdag.rand_fork_dag(V, 3, 10, seed=5)
    validators = pos.Validators(dict(zip(nodes, [(1 << 20) // (i + 1) for i in range(V)])))
    rng = np.random.default_rng(5)
    times = (1_700_000_000_000_000_000 + rng.integers(0, 10**9, len(events))).astype(np.uint64)

    ix = lx.VecfcIndex()
    ix.reset(validators)
    ix.add_events(events)
    mt = lx.MedianTimeIndex(ix)
    mt.set_times_dense(0, times)
    L, ih, mh = ix.ix.L, ix.ix.h, mt.h

    # the caller's own table: fork-free, so (validator, seq) names the event
    by = np.zeros((V, 4), dtype=np.uint64)
    for k, e in enumerate(events):
        by[validators.idxs[e.creator], e.seq] = times[k]
    w = np.array(validators.weights, dtype=np.uint64)
    vidx = np.arange(V)

    def host_medians(rows, n):
        seq = rows.view(np.uint32).reshape(n, V, 2)[:, :, 0]
        out = np.empty(n, dtype=np.uint64)
        for i in range(n):
            t = np.where(seq[i] == 0, np.uint64(args.default_time), by[vidx, seq[i]])
            order = np.argsort(t, kind="stable")
            out[i] = t[order[np.searchsorted(np.cumsum(w[order]), int(w.sum()) // 2, side="left")]]
        return out

    res = {"shape": [V, 3, 10], "events": len(events), "iters": args.iters}
    for n in (1, 256):
        ev = np.arange(len(events) - n, len(events), dtype=np.uint32)
        out = np.zeros(n, dtype=np.uint64)
        off = np.zeros(n + 1, dtype=np.uint64)
        rows = np.zeros(8 * V * n, dtype=np.uint8)
        t_mt, t_get, t_host = [], [], []
        for it in range(args.warmup + args.iters):
            t0 = time.perf_counter_ns()
            rc = L.lx_mt_median_time(mh, n, ev.ctypes.data_as(u32p), args.default_time, out.ctypes.data_as(u64p))
            t1 = time.perf_counter_ns()
            assert rc == 0, L.lx_mt_last_error(mh)
            t2 = time.perf_counter_ns()
            rc = L.lx_get_merged_highest_before_batch(ih, n, ev.ctypes.data_as(u32p), off.ctypes.data_as(u64p),
                                                      rows.ctypes.data_as(u8p), len(rows))
            t3 = time.perf_counter_ns()
            assert rc == 0 and int(off[-1]) == 8 * V * n
            ref = host_medians(rows, n)
            t4 = time.perf_counter_ns()
            assert np.array_equal(ref, out)
            if it >= args.warmup:
                t_mt.append(t1 - t0)
                t_get.append(t3 - t2)
                t_host.append(t4 - t2)

        def us(a):
            a = np.array(a) / 1e3
            return {"p50": round(float(np.percentile(a, 50)), 2), "p10": round(float(np.percentile(a, 10)), 2),
                    "p90": round(float(np.percentile(a, 90)), 2)}
        res["n%d" % n] = {"mt_us": us(t_mt), "get_merged_us": us(t_get), "get_merged_plus_numpy_us": us(t_host)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
