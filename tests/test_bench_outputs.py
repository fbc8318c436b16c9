"""bench.py --dump-outputs DIR: what the last timed step returned, as DIR/<name>.npy in float32, a fixed seeded row sample for an
output over the per-output cap; a plain run times exactly --steps steps and leaves the side measurements to --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402


def test_dump_outputs_float32_and_a_seeded_sample_of_a_large_output(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES_PER_OUTPUT", 4000)
    small = torch.arange(10, dtype=torch.float64).reshape(10, 1)
    large = torch.arange(3000, dtype=torch.float32).reshape(300, 10)          # 12 000 bytes: 100 rows of 40 bytes kept
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"probs": small, "feat": large})
    assert sorted(os.listdir(tmp_path / "a")) == ["feat_sample.npy", "probs.npy"]
    p = np.load(tmp_path / "a" / "probs.npy")
    assert p.dtype == np.float32 and np.array_equal(p, small.numpy().astype(np.float32))
    s = np.load(tmp_path / "a" / "feat_sample.npy")
    assert s.dtype == np.float32 and s.shape == (100, 10) and s.nbytes <= 4000
    rows = s[:, 0].astype(np.int64) // 10
    assert np.all(np.diff(rows) > 0) and np.array_equal(s, large.numpy()[rows])  # whole rows, in order, no repeats
    assert np.array_equal(s, np.load(tmp_path / "b" / "feat_sample.npy"))      # the same rows run after run


@pytest.mark.gpu
def test_plain_run_times_k_steps_and_dumps_the_last_step(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out)], cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["value"] > 0 and line["dtype"] == "f32"
    assert line["roofline"] is None and "cpu_baseline" not in line and "train_step" not in line     # (--full only)
    n = line["config"]["n_nodes"]
    probs = np.load(out / "probs.npy")
    assert probs.dtype == np.float32 and probs.shape == (n, 1) and np.isfinite(probs).all()
    assert ((probs > 0) & (probs < 1)).all()
    feat = np.load(out / "adj_e_features_sample.npy")
    assert feat.dtype == np.float32 and feat.nbytes <= bench.DUMP_BYTES_PER_OUTPUT and feat.shape[1] == 15
