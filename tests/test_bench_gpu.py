"""bench.py's plain run on the GPU: exactly --steps timed steps, the headline line only, and --dump-outputs writes what the
last timed step computed (its query's k results and its batch's embeddings).  A small table keeps it short."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_last_step(built, tmp_path):
    rows, steps, warmup, batch, k = 200_000, 3, 1, 256, 10
    out_dir = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                        "--rows", str(rows), "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{"metric"')]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["steps"] == steps and line["warmup"] == warmup and line["ms_per_step"] > 0
    assert line["unit"] == "images/s" and line["higher_is_better"] is True and line["dtype"] == "bf16"
    assert abs(line["value"] - batch / (line["ms_per_step"] * 1e-3)) <= 0.01 * line["value"]
    for key in ("roofline", "roofline_knn", "knn", "other_configs", "cpu_baseline", "value_single_pass_query"):
        assert key not in line, key   # --full only

    ids = np.load(out_dir / "knn_ids.npy")
    dist = np.load(out_dir / "knn_distances.npy")
    emb = np.load(out_dir / "embeddings.npy")
    assert ids.dtype == np.float64 and ids.shape == (k,)
    assert dist.dtype == np.float32 and dist.shape == (k,)
    assert emb.dtype == np.float32 and emb.shape == (batch, 768)
    assert np.all(ids == np.floor(ids)) and np.all(ids >= 0) and np.all(ids < rows + (warmup + steps) * batch)
    assert len(np.unique(ids)) == k
    assert np.all(np.isfinite(dist)) and np.all(np.diff(dist) >= 0)
    assert np.all(np.isfinite(emb)) and float(np.abs(emb).max()) > 0
