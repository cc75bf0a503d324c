#!/usr/bin/env python3
"""Latency of lx_abft_build_frames against lx_abft_build on the same handle.

On the BASELINE configs[4] shape (V = 1000 Zipf stakes, 50 events per
validator, 10 parents; the whole epoch processed first) with one candidate per
validator -- its last event plus the last events of the next nine validators:

* ``build``        : lx_abft_build of one candidate (Add, frame steps,
  DropNotFlushed: a rollback of the index);
* ``frames_n1``    : lx_abft_build_frames of the same candidate;
* ``frames_n1000`` : lx_abft_build_frames of all 1000 candidates in one call.

The three alternate inside one loop (the single candidate rotates through the
validators), host clocks around calls that end in a device synchronise, ctypes
overhead included.  Prints one JSON line (p50 / p10 / p90 in microseconds, the
per-candidate cost of the batch, and the GPU work lx_abft_build_last_stats
reports) and checks that every way gives the same frames.  Needs the GPU.
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

    out_all = np.zeros(V, dtype=np.uint32)
    root_all = np.zeros(V, dtype=np.uint8)
    out1 = np.zeros(1, dtype=np.uint32)
    root1 = np.zeros(1, dtype=np.uint8)
    off1 = np.array([0, np_], dtype=np.uint64)
    built = ctypes.c_uint32()
    err = ctypes.c_uint32()
    t_build, t_n1, t_all = [], [], []
    stats = {}
    for it in range(args.warmup + args.iters):
        i = (it * 37) % V
        pi = np.ascontiguousarray(par[i])
        t0 = time.perf_counter_ns()
        rc = L.lx_abft_build(h, int(cr[i]), int(sq[i]), np_, pi.ctypes.data_as(u32p), ctypes.byref(built))
        t1 = time.perf_counter_ns()
        assert rc == 0, L.lx_abft_last_error(h)
        t2 = time.perf_counter_ns()
        rc = L.lx_abft_build_frames(h, 1, cr[i:i + 1].ctypes.data_as(u32p), sq[i:i + 1].ctypes.data_as(u32p),
                                    off1.ctypes.data_as(u64p), pi.ctypes.data_as(u32p), out1.ctypes.data_as(u32p),
                                    root1.ctypes.data_as(u8p), ctypes.byref(err))
        t3 = time.perf_counter_ns()
        assert rc == 0, L.lx_abft_last_error(h)
        if it == args.warmup:
            stats["n1"] = lch.build_stats()
        t4 = time.perf_counter_ns()
        rc = L.lx_abft_build_frames(h, V, cr.ctypes.data_as(u32p), sq.ctypes.data_as(u32p), off.ctypes.data_as(u64p),
                                    flat.ctypes.data_as(u32p), out_all.ctypes.data_as(u32p),
                                    root_all.ctypes.data_as(u8p), ctypes.byref(err))
        t5 = time.perf_counter_ns()
        assert rc == 0, L.lx_abft_last_error(h)
        if it == args.warmup:
            stats["n%d" % V] = lch.build_stats()
        assert built.value == int(out1[0]) == int(out_all[i]), (i, built.value, int(out1[0]), int(out_all[i]))
        if it >= args.warmup:
            t_build.append(t1 - t0)
            t_n1.append(t3 - t2)
            t_all.append(t5 - t4)

    def us(a):
        a = np.array(a) / 1e3
        return {"p50": round(float(np.percentile(a, 50)), 2), "p10": round(float(np.percentile(a, 10)), 2),
                "p90": round(float(np.percentile(a, 90)), 2)}
    res = {"shape": [V, epv, P], "events": N, "iters": args.iters, "max_frame": int(frames.max()),
           "roots_among_candidates": int(root_all.sum()),
           "build_us": us(t_build), "frames_n1_us": us(t_n1), "frames_n%d_us" % V: us(t_all),
           "frames_n%d_us_per_candidate_p50" % V: round(float(np.percentile(t_all, 50)) / 1e3 / V, 3),
           "gpu_work": stats}
    print(json.dumps(res))
    lch.close()


if __name__ == "__main__":
    main()
