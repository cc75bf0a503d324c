"""Walk cycles of the headline config (C3: V = 1000, Zipf stakes, 10M events,
one batch, default options) with whichever library LX_LIB names: per index
step the walk's shader cycles (lx_last_walk_clock: median clock x the median
workgroup's walk, as bench.py's walk_clock.walk_mcycles_median) beside the
walk and index times.  The cycle count is set by the code and the DAG, not by
the clock the box grants, so it is what a walker A/B compares;
one JSON line per process.  WT_OPTS: index options as JSON."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "lachesis-base_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import lachesis_hip as lx  # noqa: E402

V, epv = int(os.environ.get("WT_V", "1000")), int(os.environ.get("WT_EPV", "10000"))
d = lx.tools.gen_dag(V, epv, 10, seed=1)
N = len(d)
w = [(1 << 20) // (i + 1) for i in range(V)]
dev = torch.device("cuda", 0)
to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(dev)
dc, ds, dp, do = to_dev(d.creator), to_dev(d.seq), to_dev(d.par), to_dev(d.poff.astype(np.uint32))
ix = lx.Index(event_capacity=N, options=json.loads(os.environ.get("WT_OPTS", "{}")))
ks, walks, mcyc, mhz = [], [], [], []
for r in range(int(os.environ.get("WT_STEPS", "5")) + 1):
    ix.reset(w)
    ix.add_batch_dev(N, dc.data_ptr(), ds.data_ptr(), do.data_ptr(), dp.data_ptr())
    ix.sync()
    ks.append(round(ix.last_stats()["ms_index"], 3))
    st = ix.segment_stats()
    walks.append(round(max(st["walk_ms"]), 3) if st["segments"] else None)
    c = ix.walk_clock()
    mhz.append(round(c["mhz_median"], 1))
    mcyc.append(round(c["mhz_median"] * c["walk_ms"] / 1e3, 3))
print(json.dumps({"lib": os.environ.get("LX_LIB", "build/liblachesis_hip.so"), "opts": os.environ.get("WT_OPTS", "{}"),
                  "events": N, "walk_mcycles_min": min(mcyc[1:]), "walk_mcycles_median": float(np.median(mcyc[1:])),
                  "walk_mcycles": mcyc[1:], "mhz": mhz[1:], "walk_ms": walks[1:], "ms_index": ks[1:],
                  "segments": ix.segment_stats()["segments"],
                  # partial events per segment: a walk that publishes wrong rows shows up here
                  "partial": ix.segment_stats()["partial"]}))
