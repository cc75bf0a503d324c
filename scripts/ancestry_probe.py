#!/usr/bin/env python3
"""Time of lx_anc_confirm against the library's own host walk.

On the BASELINE configs[4] shape (V = 1000, Zipf stakes, 50 events per
validator, 10 parents, no cheaters: bench.py's abft leg) one epoch is run
through lx_abft_process_batch under block_log 2; its blocks give the Atropoi.
Every iteration then measures, one after the other:

* ``host_walk``      : the epoch again with claimed frames; the figures are
  ``lx_abft_last_stats.ms_blocks`` and ``ms_election``.  The library does not
  fill ``ms_blocks`` (it reads 0): the block phase -- cheaters, the stack walk
  over the host parent lists for every block, the block log -- is timed inside
  ``ms_election`` together with the votes and decisions, so ``ms_election``
  bounds the host walk from above and is no measurement of it.  This work
  leaves that code as it is;
* ``anc_per_block``  : lx_anc_confirm, one block per call, over all blocks of
  the epoch on a handle without labels (per call and summed);
* ``anc_one_call``   : lx_anc_confirm with all of the epoch's Atropoi in one
  call on a handle without labels.

The lx_anc figures are host clocks around calls that end in a device
synchronise, ctypes overhead included.  Checks that the three give the same
number of events per block.  Prints one JSON line (p50 / p10 / p90).  Needs
the GPU.
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

u32p = ctypes.POINTER(ctypes.c_uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--validators", type=int, default=1000)
    ap.add_argument("--events-per-validator", type=int, default=50)
    args = ap.parse_args()

    import lachesis_hip as lx

    V, epv, P = args.validators, args.events_per_validator, 10
    weights = np.array([(1 << 20) // (i + 1) for i in range(V)], dtype=np.uint32)
    dag = lx.tools.gen_dag(V, epv, P, 0, 0, seed=1)
    N = len(dag)
    lch = lx.abft.DenseLachesis(weights, event_capacity=N, apply_events=True, block_log=True)
    rc, consumed, frames = lch.process_batch(dag.creator, dag.seq, dag.poff, dag.par)
    assert rc == 0 and consumed == N
    blocks = list(lch.blocks)
    heads = np.array([b[2] for b in blocks], dtype=np.uint32)
    labels = np.array([b[1] for b in blocks], dtype=np.uint32)
    want = np.array([len(b[4]) for b in blocks], dtype=np.uint32)
    nb = len(blocks)
    assert nb > 0

    class _Dagi:
        ix, ids = lch.ix, range(N)
    anc = lx.ancestry.AncestryIndex(_Dagi)
    L, ah = anc.L, anc.h
    n_new = np.zeros(nb, dtype=np.uint32)

    t_host, t_elect, t_call, t_sum, t_one = [], [], [], [], []
    for it in range(args.warmup + args.iters):
        # the epoch again: the index is reset, the ancestry handle follows it
        L.lx_abft_reset(lch.h, 1, V, weights.ctypes.data_as(u32p))
        lch.blocks = []
        rc, consumed, _ = lch.process_batch(dag.creator, dag.seq, dag.poff, dag.par, frames)
        assert rc == 0 and consumed == N and len(lch.blocks) == nb
        st = lch.last_stats()
        host_ms, elect_ms = st["ms_blocks"], st["ms_election"]
        assert anc.low_water() == 0

        calls = []
        for k in range(nb):
            t0 = time.perf_counter_ns()
            rc = L.lx_anc_confirm(ah, 1, heads[k:].ctypes.data_as(u32p), labels[k:].ctypes.data_as(u32p),
                                  n_new[k:].ctypes.data_as(u32p))
            calls.append(time.perf_counter_ns() - t0)
            assert rc == 0, L.lx_anc_last_error(ah)
        assert np.array_equal(n_new, want)

        anc.reset()
        n_new[:] = 0
        t0 = time.perf_counter_ns()
        rc = L.lx_anc_confirm(ah, nb, heads.ctypes.data_as(u32p), labels.ctypes.data_as(u32p),
                              n_new.ctypes.data_as(u32p))
        one = time.perf_counter_ns() - t0
        assert rc == 0 and np.array_equal(n_new, want)
        if it >= args.warmup:
            t_host.append(host_ms)
            t_elect.append(elect_ms)
            t_call += [c / 1e3 for c in calls]
            t_sum.append(sum(calls) / 1e6)
            t_one.append(one / 1e6)

    def pct(a):
        return {"p50": round(float(np.percentile(a, 50)), 3), "p10": round(float(np.percentile(a, 10)), 3),
                "p90": round(float(np.percentile(a, 90)), 3)}
    print(json.dumps({"shape": [V, epv, P], "events": N, "blocks": nb, "confirmed": int(want.sum()),
                      "iters": args.iters,
                      "host_walk_ms_blocks": pct(t_host), "host_ms_election": pct(t_elect),
                      "anc_per_block_call_us": pct(t_call),
                      "anc_per_block_epoch_ms": pct(t_sum), "anc_one_call_ms": pct(t_one)}))


if __name__ == "__main__":
    main()
