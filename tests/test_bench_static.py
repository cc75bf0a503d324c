"""bench.py runs only on a GPU box: catch names a leg uses but never binds
(a NameError there costs a whole GPU call) with a static scan on the CPU."""

import ast
import builtins
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bound(node):
    out = set()
    for n in ast.walk(node):
        if isinstance(n, ast.Name) and isinstance(n.ctx, (ast.Store, ast.Del)):
            out.add(n.id)
        elif isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef, ast.ClassDef)):
            out.add(n.name)
        elif isinstance(n, ast.arg):
            out.add(n.arg)
        elif isinstance(n, (ast.Import, ast.ImportFrom)):
            out.update((a.asname or a.name).split(".")[0] for a in n.names)
        elif isinstance(n, ast.ExceptHandler) and n.name:
            out.add(n.name)
        elif isinstance(n, (ast.Global, ast.Nonlocal)):
            out.update(n.names)
    return out


def test_bench_functions_bind_every_name_they_use():
    tree = ast.parse(open(os.path.join(ROOT, "bench.py"), encoding="utf-8").read())
    module = set(dir(builtins)) | {"__file__", "__name__"}
    for n in tree.body:
        module |= _bound(n) if not isinstance(n, (ast.FunctionDef, ast.ClassDef)) else {n.name}
    bad = []
    for f in tree.body:
        if not isinstance(f, ast.FunctionDef):
            continue
        known = module | _bound(f)
        for n in ast.walk(f):
            if isinstance(n, ast.Name) and isinstance(n.ctx, ast.Load) and n.id not in known:
                bad.append((f.name, n.id, n.lineno))
    assert not bad, bad


def test_dump_helpers(tmp_path):
    """--dump-outputs: the sample is fixed, the files are float32 where that is
    exact and float64 otherwise, rows of one length come out as a matrix."""
    import numpy as np
    import bench
    s = bench.dump_sample(10_000_000, 1024)
    assert np.array_equal(s, bench.dump_sample(10_000_000, 1024))
    assert len(np.unique(s)) == 1024 and (np.diff(s) > 0).all() and 0 <= s[0] and s[-1] < 10_000_000
    assert np.array_equal(bench.dump_sample(7, 1024), np.arange(7))
    d = str(tmp_path)
    bench.save_npy(d, "small", np.array([0, (1 << 24) - 1], dtype=np.uint32))
    bench.save_npy(d, "large", np.array([0, (1 << 24) + 1], dtype=np.uint32))
    small, large = np.load(os.path.join(d, "small.npy")), np.load(os.path.join(d, "large.npy"))
    assert small.dtype == np.float32 and small[1] == (1 << 24) - 1
    assert large.dtype == np.float64 and large[1] == (1 << 24) + 1
    words = np.arange(6, dtype=np.uint32)
    bench.save_rows(d, "even", np.array([0, 12, 24], dtype=np.uint64), words.view(np.uint8))
    assert np.array_equal(np.load(os.path.join(d, "even.npy")), words.reshape(2, 3))
    bench.save_rows(d, "ragged", np.array([0, 8, 24], dtype=np.uint64), words.view(np.uint8))
    assert np.array_equal(np.load(os.path.join(d, "ragged.npy")), words)
    assert np.array_equal(np.load(os.path.join(d, "ragged_offsets.npy")), [0, 2, 6])


def test_plain_run_gates_every_other_leg():
    """Whatever bench.py measures beside the headline runs under --full only:
    every call of such a leg in main() sits under a condition that names
    args.full."""
    tree = ast.parse(open(os.path.join(ROOT, "bench.py"), encoding="utf-8").read())
    main = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "main")
    legs = {"latency_leg", "feed_levels", "qi_leg", "config_leg", "abft_leg", "dropin_leg", "cpu_baseline",
            "power_probe"}
    seen = set()

    def walk(node, gated):
        if isinstance(node, ast.If):
            g = gated or any(isinstance(n, ast.Attribute) and n.attr == "full" for n in ast.walk(node.test))
            for c in node.body:
                walk(c, g)
            for c in node.orelse:
                walk(c, gated)
            return
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id in legs:
            assert gated, (node.func.id, node.lineno)
            seen.add(node.func.id)
        for c in ast.iter_child_nodes(node):
            walk(c, gated)

    walk(main, False)
    assert seen == legs, legs - seen


def test_multi_gpu_line_keys():
    """The committed N = 2 rehearsal line (two ranks over gloo on one GPU,
    scripts/rowseg_rehearsal.sh; the driver's N > 1 runs use RCCL) carries what
    the N > 1 bench line must: the k_fc roofline computed the N = 1 way from
    the early-exit counters summed over the ranks (frac < 1), k_fc timed
    apart from the routing protocol, per-rank device bytes, and both the
    row-segment block and the column-shard block of BASELINE configs[2]."""
    import glob
    import json
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*", "rehearsal", "rowseg_colshard_g2*.json")))
    assert files, "no committed N=2 rehearsal line"
    r = json.loads(open(files[-1]).read().strip().splitlines()[-1])
    assert r["n_gpus"] == 2 and r["config"]["parallelism"] == "rowseg2"
    roof = r["roofline"]
    assert roof["early_exit"] is not None and roof["early_exit"]["queries"] > 0
    assert roof["early_exit"]["answered"] == 2 * r["steps"] * r["config"]["fc_queries"]
    assert 0 < roof["frac"] < 1 and roof["bytes_read_per_launch"] < roof["algorithmic_bytes_per_launch"]
    assert "whole_row_equiv_frac" in roof
    rs = r["rowseg"]
    assert rs["fc_kernel_ms"] > 0 and rs["fc_protocol_ms"] > 0
    # the protocol split into the library's device steps and the collectives (round 6)
    assert rs["fc_protocol_device_ms"] > 0 and rs["fc_protocol_collective_ms"] > 0
    assert rs["fc_protocol_device_ms"] + rs["fc_protocol_collective_ms"] <= rs["fc_protocol_ms"] * 1.05
    assert abs(rs["fc_kernel_ms"] + rs["fc_protocol_ms"] - rs["fc_step_ms"]) < 1e-6 * rs["fc_step_ms"] + 1e-9
    cs = r["colshard"]
    assert cs["events_per_sec"] > 0 and cs["fc_queries_per_sec"] > 0 and cs["exchange_ms"] is not None
    assert 0 < cs["roofline"]["frac"] < 1
    # a rank's planes hold its own rows: half of the epoch's at N = 2
    rows = rs["rows"][1] - rs["rows"][0]
    assert r["device_bytes_per_rank"]["planes"] <= 8 * rows * 1088 + 1
