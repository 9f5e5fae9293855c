"""The plain bench run (`python bench.py --gpus N --steps K --warmup W`, no --full): ONE JSON line with the headline figure only
(configs[3] retrieve + rerank), exactly K timed steps, and with --dump-outputs DIR the last timed batch's outputs as DIR/<name>.npy in
float32 / float64. The --full line is guarded by tests/test_bench_two_ranks_gpu.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HEADLINE_KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY_KEYS = ("p50_batch_latency_ms", "roofline", "cpu_baseline", "dense", "hybrid", "agent_latency", "shard_12p5M")


def test_dump_outputs_writes_float32_and_float64(tmp_path):
    import bench
    ids = np.array([[0, 2 ** 40 + 1], [7, 3]], dtype=np.int64)
    bench.dump_outputs(str(tmp_path / "out"), {"ids": ids, "scores": np.array([0.5, 0.25]), "logits": np.array([1.5], dtype=np.float32)})
    got = {n: np.load(tmp_path / "out" / (n + ".npy")) for n in ("ids", "scores", "logits")}
    assert got["ids"].dtype == np.float64 and (got["ids"].astype(np.int64) == ids).all()
    assert got["scores"].dtype == np.float64 and got["logits"].dtype == np.float32 and got["logits"][0] == 1.5


def _plain_run(tmp_path, gpus, extra_env=None):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(extra_env or {})
    out = tmp_path / "outputs"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(gpus), "--steps", "2", "--warmup", "1", "--rows", "250000",
                        "--dump-outputs", str(out)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, (p.returncode, p.stderr[-3000:])
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    for key in HEADLINE_KEYS:
        assert d[key] is not None, key
    assert "retrieve+rerank" in d["metric"] and d["unit"] == "queries/sec" and d["higher_is_better"] is True
    assert d["n_gpus"] == gpus and d["steps"] == 2 and d["warmup"] == 1 and d["value"] > 0 and d["ms_per_step"] > 0
    assert abs(d["value"] - 256 / (d["ms_per_step"] * 1e-3)) / d["value"] < 0.01        # one step = one 256-query batch
    assert d["config"]["corpus_rows"] == 250000 and d["config"]["batch_queries"] == 256
    for key in FULL_ONLY_KEYS:
        assert key not in d, key
    o = {n: np.load(out / (n + ".npy")) for n in ("ids", "scores", "logits", "candidates")}
    assert o["ids"].shape == (256, 20) and o["scores"].shape == (256, 20) and o["logits"].shape == (256, 20)
    assert o["candidates"].shape == (256, 100)
    assert o["ids"].dtype == o["scores"].dtype == o["candidates"].dtype == np.float64 and o["logits"].dtype == np.float32
    ids = o["ids"].astype(np.int64)
    assert (ids == o["ids"]).all() and (ids >= 0).all() and (ids < 250000).all()
    assert (o["scores"][:, :-1] >= o["scores"][:, 1:]).all()
    assert all(set(ids[i]) <= set(o["candidates"][i].astype(np.int64)) for i in range(256))
    return d


@pytest.mark.gpu
def test_plain_line_one_gpu(tmp_path):
    d = _plain_run(tmp_path, 1)
    assert d["config"]["exchange"] == "single process"


@pytest.mark.gpu
def test_plain_line_two_ranks_on_one_gpu(tmp_path):
    """The N > 1 plain path (ShardedPipeline), both ranks on cuda:0 with collectives through gloo."""
    d = _plain_run(tmp_path, 2, {"RAG_BENCH_BACKEND": "gloo"})
    assert "gloo" in d["config"]["exchange"] and d["config"]["rows_per_gpu"] == 125000
