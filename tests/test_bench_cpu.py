"""CPU: the bench harness's own helpers (no GPU): the oracle-based CPU baseline must return the exact intersection for
any shard count, since bench.py cross-checks the GPU result against it."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cpu_baseline_intersect_sharded_equals_numpy():
    b = _bench()
    rng = np.random.default_rng(3)
    lists = [np.unique(rng.integers(0, 400_000, n)).astype(np.uint32) for n in (120_000, 90_000)]
    want = np.intersect1d(lists[0], lists[1], assume_unique=True)
    removed = want[::5].copy()
    for threads in (1, 3, 8):
        rate, res, per = b.cpu_baseline_intersect(lists, None, 1, threads=threads)
        assert np.array_equal(res, want) and rate > 0 and per > 0
        _, res2, _ = b.cpu_baseline_intersect(lists, removed, 1, threads=threads)
        assert np.array_equal(res2, np.setdiff1d(want, removed, assume_unique=True))


def test_bench_argument_contract():
    b = _bench()
    import sys
    argv = sys.argv
    try:
        sys.argv = ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"]
        a = b.parse()
    finally:
        sys.argv = argv
    assert (a.gpus, a.steps, a.warmup, a.workload) == (1, 7, 2, "all")
    assert a.full is False and a.dump_outputs is None          # a plain run times the headline alone, dumps nothing


def test_secondary_workloads_need_full():
    import sys

    import pytest
    b = _bench()
    argv = sys.argv
    try:
        sys.argv = ["bench.py", "--full", "--workload", "strong", "--dump-outputs", "d"]
        with pytest.raises(SystemExit):
            b.parse()                                          # the dump is the headline's
        sys.argv = ["bench.py", "--workload", "merge"]
        with pytest.raises(SystemExit):
            b.parse()
        sys.argv = ["bench.py", "--full", "--workload", "merge"]
        assert b.parse().full
        sys.argv = ["bench.py", "--workload", "intersect", "--dump-outputs", "d"]
        assert b.parse().dump_outputs == "d"
    finally:
        sys.argv = argv


def test_intersect_dump_is_exact_seeded_and_bounded(tmp_path):
    """--dump-outputs: float64 arrays, every sampled id exact, the same sample on every run, at most 64 MB in all."""
    b = _bench()
    rng = np.random.default_rng(9)
    ids = np.sort(rng.choice(100_000_000, b.DUMP_SAMPLE_IDS + 12_345, replace=False)).astype(np.uint32)
    d = b.intersect_dump(ids)
    assert all(v.dtype == np.float64 for v in d.values())
    assert sum(v.nbytes for v in d.values()) <= 64 << 20
    assert int(d["intersect_count"][0]) == ids.size and d["intersect_ids"].size == b.DUMP_SAMPLE_IDS
    pos = d["intersect_ids_pos"].astype(np.int64)
    assert np.all(np.diff(pos) > 0) and np.array_equal(d["intersect_ids"].astype(np.uint32), ids[pos])
    assert d["intersect_ids_sum"][0] == float(ids.astype(np.uint64).sum())
    d2 = b.intersect_dump(ids.copy())
    assert all(np.array_equal(d[k], d2[k]) for k in d)
    small = b.intersect_dump(ids[:1000])
    assert np.array_equal(small["intersect_ids"], ids[:1000].astype(np.float64))
    b.dump_outputs(str(tmp_path / "out"), small)
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == sorted(k + ".npy" for k in small)
    assert np.array_equal(np.load(tmp_path / "out" / "intersect_ids.npy"), small["intersect_ids"])


def test_gpus_n_starts_n_ranks():
    """`bench.py --gpus 2` without a launcher starts two ranks itself (torch.distributed.run on 127.0.0.1) before touching a
    GPU; --dry-run keeps the ranks off the GPU: they join a gloo group, count themselves and rank 0 prints the frame."""
    import json
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--dry-run"],
                         capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1                                   # rank 0 alone prints
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["ranks_counted"] == 2 and rec["steps"] == 3 and rec["dry_run"] is True


def test_c5_index_is_the_same_for_any_rank_count():
    """configs[4]'s lists are defined on 8 fixed doc shards: 1, 2, 4 and 8 ranks hold the same index."""
    b = _bench()
    D = 4_000_000
    whole, _ = b.c5_lists(D, 1, 0)
    for world in (2, 8):
        parts = [b.c5_lists(D, world, r) for r in range(world)]
        for t in range(len(b.C5_RANKS)):
            cat = np.concatenate([p[0][t] for p in parts])
            assert np.array_equal(cat, whole[t])
        assert [p[1] for p in parts] == [(r * D // world, (r + 1) * D // world) for r in range(world)]
    core = np.unique(np.random.default_rng(55).integers(0, D, 10_000)).astype(np.uint32)
    assert all(np.isin(core, l).all() for l in whole)
