"""bench.py's command line: a plain run times the headline step alone (everything else is behind --full), and
--dump-outputs writes what the last timed step computed as float32 .npy files within a 64 MB budget."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_is_the_default(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "20", "--warmup", "5")
    assert a.full is False and a.dump_outputs is None
    assert a.steps == 20 and a.warmup == 5 and a.steps_per_graph == 20
    a = _parse(monkeypatch, "--steps", "30", "--full", "--dump-outputs", "out")
    assert a.full is True and a.dump_outputs == "out" and 30 % a.steps_per_graph == 0


def test_dump_writes_float32_and_keeps_float64(tmp_path):
    bench.dump_outputs(str(tmp_path), {"pred": torch.arange(6, dtype=torch.float16).view(2, 3),
                                       "loss": torch.tensor(0.25), "ref": torch.ones(4, dtype=torch.float64)})
    assert sorted(os.listdir(tmp_path)) == ["loss.npy", "pred.npy", "ref.npy"]
    pred = np.load(tmp_path / "pred.npy")
    assert pred.dtype == np.float32 and pred.shape == (2, 3) and pred[1, 2] == 5.0
    assert np.load(tmp_path / "loss.npy").dtype == np.float32 and float(np.load(tmp_path / "loss.npy")) == 0.25
    assert np.load(tmp_path / "ref.npy").dtype == np.float64


def test_dump_samples_a_large_output_the_same_way_every_time(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4096)
    big = torch.arange(10_000, dtype=torch.float32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": torch.zeros(8)})
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert np.load(tmp_path / "a" / "small.npy").shape == (8,)                        # fits: written whole
    assert a.nbytes + 32 <= 4096 and a.nbytes > 2048 and np.array_equal(a, b)
    assert np.all(np.diff(a) > 0) and set(a.astype(np.int64)) <= set(range(10_000))   # sorted elements of the output
    bench.dump_outputs(str(tmp_path / "c"), {"x": torch.ones(512), "y": torch.ones(256)})  # 3 KB: nothing sampled
    assert np.load(tmp_path / "c" / "x.npy").shape == (512,) and np.load(tmp_path / "c" / "y.npy").shape == (256,)


@pytest.mark.gpu
def test_plain_line_and_dumped_outputs(tmp_path):
    out = tmp_path / "dump"
    pr = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "6", "--warmup", "2",
                         "--dump-outputs", str(out)], cwd=ROOT, stdout=subprocess.PIPE, timeout=600)
    assert pr.returncode == 0
    lines = pr.stdout.decode().strip().splitlines()
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 6 and d["warmup"] == 2 and d["full"] is False and d["n_gpus"] == 1
    assert d["unit"] == "graphs/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["ms_per_step"] > 0 and abs(d["value"] - 128 / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    for k in ("roofline", "cpu_baseline", "repeats", "other_cluster_ids", "stage_a", "stage_a_dense",
              "streaming_spmm_scaled", "one_step_per_graph"):
        assert d[k] is None, k
    files = sorted(os.listdir(out))
    assert {"pred.npy", "score.npy", "loss.npy"} <= set(files) and any(f.startswith("grad.") for f in files)
    pred, score = np.load(out / "pred.npy"), np.load(out / "score.npy")
    assert pred.dtype == np.float32 and pred.shape == (128, 10) and np.isfinite(pred).all()
    np.testing.assert_allclose(score, 1.0 / (1.0 + np.exp(-pred)), rtol=1e-5, atol=1e-6)
    assert sum(os.path.getsize(out / f) for f in files) <= 64 << 20
