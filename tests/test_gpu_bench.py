"""bench.py's plain run and --dump-outputs on the smallest config (C1: 5
validators, 5,000 events): the line carries the headline keys, --steps sets
the timed steps, the legs of --full stay out, and the dumped arrays are the
oracle's rows and answers, identical from run to run."""

import json
import os
import sys

import numpy as np
import pytest

from oracle import corc

pytestmark = pytest.mark.gpu

FULL_ONLY = ("latency", "quorum_indexer", "configs", "abft", "dropin_c5", "cpu_baseline", "colshard")
FC_N = 4096


def _run(monkeypatch, capsys, out_dir):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1", "--config", "c1",
                                      "--fc-queries", str(FC_N), "--dump-outputs", str(out_dir)])
    bench.main()
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    arrays = {f[:-4]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}
    return line, arrays


def test_plain_run_line_and_dumped_outputs(monkeypatch, capsys, tmp_path):
    import bench
    import lachesis_hip as lx
    r, a = _run(monkeypatch, capsys, tmp_path / "a")
    V, epv, P, ch, fk, wkind = bench.CONFIGS["c1"]
    N = V * epv
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in r, k
    assert r["steps"] == 2 and r["warmup"] == 1 and r["unit"] == "events/s" and r["higher_is_better"] is True
    assert r["ms_per_step"] > 0 and r["value"] == pytest.approx(N / (r["ms_per_step"] * 1e-3), rel=1e-9)
    assert r["fc_queries_per_sec"] > 0
    assert not [k for k in FULL_ONLY if k in r]
    assert r["walk_power"] is None and r["fc_spot_checked"] == 0

    assert sorted(a) == ["fc_query_sample", "forkless_cause", "highest_before", "lowest_after", "row_events"]
    assert all(x.dtype in (np.float32, np.float64) for x in a.values())
    assert sum(x.nbytes for x in a.values()) <= 64e6
    # the same workload through the oracle
    d = lx.tools.gen_dag(V, epv, P, ch, fk, seed=1)
    w = bench.weights_for(V, wkind)
    o = corc.OracleIndex(w)
    assert o.add_batch(d.creator, d.seq, d.poff, d.par) == -1
    ev = a["row_events"].astype(np.int64)
    assert len(ev) == bench.DUMP_ROW_EVENTS and len(np.unique(ev)) == len(ev) and ev.min() >= 0 and ev.max() < N
    for name, row in (("highest_before", o.hb), ("lowest_after", o.la)):
        want = np.stack([np.frombuffer(row(int(e)), dtype=np.uint32) for e in ev])
        assert np.array_equal(a[name], want), name
    qa, qb = lx.tools.fc_queries(d.lamport, FC_N, window=64, seed=7)
    qs = a["fc_query_sample"].astype(np.int64)
    assert np.array_equal(qs, np.arange(FC_N))   # fewer queries than the sample size: all of them
    assert np.array_equal(a["forkless_cause"], o.forkless_cause_batch(qa[qs], qb[qs]))

    # the same arguments again: the same inputs, the same outputs
    _, b = _run(monkeypatch, capsys, tmp_path / "b")
    assert sorted(b) == sorted(a)
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
