"""Batched ForklessCause in a fork epoch with and without the early exit
(option fc_early_forks: k_fc_fk_early against k_fc_fk) on the C3 shape
(V = 1000, Zipf stakes, 10M events) with 1 and with 3 light cheaters, 2^24
queries of the bench's shape (b within 64 Lamport of a), device arrays.  The
two settings alternate in one process, every launch timed by device events,
answers compared byte for byte; the fork-free epoch's k_fc_early on the same
box goes beside them for scale.  Reports the round counters and the bytes of
row data each path reads by the model (16 B per uint4 of HB(a) and LA(b)).
Prints one JSON line and, with a path argument, writes it there."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "lachesis-base_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import lachesis_hip as lx  # noqa: E402

V, epv = int(os.environ.get("FE_V", "1000")), int(os.environ.get("FE_EPV", "10000"))
NQ = 1 << int(os.environ.get("FE_LOGQ", "24"))
REPS, PASSES = 5, 3
w = [(1 << 20) // (i + 1) for i in range(V)]
dev = torch.device("cuda", 0)
to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(dev)


def timed(ix, ta, tb, out):
    """One launch between two device events, ms."""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    ix.forkless_cause_batch_dev(NQ, ta.data_ptr(), tb.data_ptr(), out.data_ptr())
    ix.sync()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def run(cheaters):
    d = lx.tools.gen_dag(V, epv, 10, cheaters=cheaters, forks=3, seed=1)
    d.creator = (V - 1 - d.creator.astype(np.int64)).astype(np.uint32)   # the cheaters are the lightest validators
    N = len(d)
    dc, ds, dp, do = to_dev(d.creator), to_dev(d.seq), to_dev(d.par), to_dev(d.poff.astype(np.uint32))
    ix = lx.Index(event_capacity=N)
    ix.reset(w)
    ix.add_batch_dev(N, dc.data_ptr(), ds.data_ptr(), do.data_ptr(), dp.data_ptr())
    ix.sync()
    B = ix.num_branches()
    qa, qb = lx.tools.fc_queries(d.lamport, NQ, window=64, seed=7)
    ta, tb = to_dev(qa), to_dev(qb)
    res = {"cheaters": cheaters, "events": N, "branches": B}
    out = torch.empty(NQ, dtype=torch.uint8, device=dev)
    if not cheaters:
        assert B == V
        ts = [timed(ix, ta, tb, out) for _ in range(1 + REPS * PASSES)][1:]
        res["ms_fc_early"] = float(np.median(ts))
        res["rounds_fc_early"] = ix.fc_early_rounds()
        ix.close()
        return res
    assert B > V
    ms, outs = {0: [], 1: []}, {}
    for opt in (1, 0):                                   # warm both kernels up
        ix.set_option("fc_early_forks", opt)
        timed(ix, ta, tb, out)
    ix.fc_early_fork_rounds()
    for _ in range(PASSES):                              # alternate the settings
        for opt in (0, 1):
            ix.set_option("fc_early_forks", opt)
            ms[opt].append(float(np.median([timed(ix, ta, tb, out) for _ in range(REPS)])))
            outs[opt] = out.cpu().numpy()
    r = ix.fc_early_fork_rounds()
    launches = REPS * PASSES
    assert all(x % launches == 0 for x in r) and r[2] == NQ * launches
    r = [x // launches for x in r]
    t0, hi4 = V // 4, (B + 3) // 4
    per_round = [32 + hi4 - t0, 32, 64, t0 - 128]        # uint4 of one row
    read = sum(n * u for n, u in zip([NQ, r[0], r[1], r[3]], per_round)) * 32
    res.update({"ms_fc_fk": ms[0], "ms_fc_fk_early": ms[1],
                "ms_fc_fk_median": float(np.median(ms[0])), "ms_fc_fk_early_median": float(np.median(ms[1])),
                "speedup": float(np.median(ms[0]) / np.median(ms[1])),
                "identical": bool(np.array_equal(outs[0], outs[1])), "true_frac": float(outs[0].mean()),
                "fork_rounds": {"past_round1": r[0], "past_round2": r[1], "queries": r[2], "past_round3": r[3]},
                "model_bytes_fc_fk": NQ * hi4 * 32, "model_bytes_fc_fk_early": read,
                "model_GBps_fc_fk": NQ * hi4 * 32 / np.median(ms[0]) / 1e6,
                "model_GBps_fc_fk_early": read / np.median(ms[1]) / 1e6})
    ix.close()
    return res


result = {"V": V, "events_per_validator": epv, "zipf": True, "queries": NQ, "window": 64,
          "timing": "device events around one launch + sync; median of %d launches per pass, %d alternating passes"
                    % (REPS, PASSES),
          "runs": []}
for c in (1, 3, 0):
    result["runs"].append(run(c))
    print("done: %d cheaters" % c, file=sys.stderr, flush=True)
line = json.dumps(result)
print(line)
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w", encoding="utf-8") as f:
        f.write(json.dumps(result, indent=1) + "\n")
