"""bench.py's command line: `--dump-outputs DIR` writes what the last timed step returned as float32 .npy files (a seeded
sample of rows past the size budget), and a plain run times the steps and nothing else (`roofline` and `cpu_baseline` are
null, no side file): the runs of their own are behind `--full`."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]


def test_dump_outputs_writes_float32_and_samples_the_same_rows_of_every_array(tmp_path):
    code = ("import sys, torch, bench\n"
            "g = torch.Generator().manual_seed(1)\n"
            "arrays = dict(out=torch.randn((40, 64), generator=g).to(torch.bfloat16), topk_weights=torch.rand((40, 2), generator=g),\n"
            "              topk_ids=torch.randint(0, 8, (40, 2), generator=g, dtype=torch.int32))\n"
            "torch.save(arrays, sys.argv[1] + '/arrays.pt')\n"
            "bench.dump_outputs(sys.argv[1] + '/whole', arrays, 0, 1)\n"
            "bench.DUMP_BYTES = 2 * 10 * (64 + 2 + 2) * 4 + 7      # two ranks, ten rows each and a little\n"
            "bench.dump_outputs(sys.argv[1] + '/part', arrays, 1, 2)\n")
    r = subprocess.run([sys.executable, "-c", code, str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    import torch
    arrays = torch.load(tmp_path / "arrays.pt")
    assert sorted(p.name for p in (tmp_path / "whole").iterdir()) == ["out.npy", "topk_ids.npy", "topk_weights.npy"]
    for k, t in arrays.items():
        a = np.load(tmp_path / "whole" / f"{k}.npy")
        assert a.dtype == np.float32 and np.array_equal(a, t.float().numpy()), k
    rows = np.load(tmp_path / "part" / "sampled_rows_rank1.npy")
    assert rows.dtype == np.float64 and len(rows) == 10 and len(set(rows)) == 10 and np.all(np.diff(rows) > 0)
    total = 0
    for k, t in arrays.items():
        a = np.load(tmp_path / "part" / f"{k}_rank1.npy")
        assert a.dtype == np.float32 and np.array_equal(a, t.float().numpy()[rows.astype(int)]), k
        total += a.nbytes
    assert 2 * total <= 2 * 10 * (64 + 2 + 2) * 4 + 7


@pytest.mark.gpu
def test_plain_run_times_the_steps_dumps_them_and_leaves_the_rest_to_full(tmp_path):
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2",
           "--full-out", str(tmp_path / "side.json"), "--dump-outputs", str(tmp_path / "dump")]
    r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1                                   # no extra workloads
    j = json.loads(lines[0])
    assert j["metric"] == "moe_layer_decode_tokens_per_s" and j["unit"] == "tokens/s" and j["higher_is_better"] is True
    assert j["steps"] == 5 and j["dtype"] == "bf16" and j["ms_per_step"] > 0
    M = j["config"]["batch_per_gpu"]
    assert j["value"] == pytest.approx(M / (j["ms_per_step"] * 1e-3), rel=1e-3)
    assert j["roofline"] is None and j["cpu_baseline"] is None and "long_run" not in j
    assert not (tmp_path / "side.json").exists()
    out, tw, ids = (np.load(tmp_path / "dump" / f"{k}.npy") for k in ("out", "topk_weights", "topk_ids"))
    K, E, H = j["config"]["top_k"], j["config"]["experts"], j["config"]["hidden"]
    assert out.dtype == tw.dtype == ids.dtype == np.float32
    assert out.shape == (M, H) and tw.shape == ids.shape == (M, K)
    assert np.isfinite(out).all() and np.abs(out).max() > 0
    assert np.array_equal(ids, np.round(ids)) and ids.min() >= 0 and ids.max() < E
    np.testing.assert_allclose(tw.sum(axis=1), 1.0, rtol=1e-5)      # renormalised top-k weights
