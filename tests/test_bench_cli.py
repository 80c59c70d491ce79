"""bench.py's two kinds of run: a plain run (the default) does only what its headline figure needs and writes --dump-outputs;
--full adds the per-kernel, parity, secondary and CPU-baseline legs (too slow for the suite: not run here)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "kernels", "top_mfma_kernel", "data_parallel", "modes", "variants", "eval_path", "cpu_baseline")


def test_full_is_off_by_default():
    assert bench.parse_args([]).full is False
    assert bench.parse_args(["--full", "--no-cpu-baseline"]).full is True
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert (a.gpus, a.steps, a.warmup, a.dump_outputs) == (1, 7, 3, None)


@pytest.mark.gpu
def test_plain_run_prints_the_headline_only_and_dumps(tmp_path):
    steps, warmup, users = 3, 1, 512
    dump = tmp_path / "dump"
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                        "--resident-batches", "2", "--dump-outputs", str(dump)],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    for k in HEADLINE:
        assert k in out, k
    assert out["unit"] == "users/s" and out["higher_is_better"] is True and out["dtype"] == bench.DTYPES["fp16"]
    assert out["steps"] == steps and out["warmup"] == warmup and out["warmup_effective"] == 1 + 2 * steps + warmup
    assert out["value"] > 0 and out["ms_per_step"] > 0
    assert abs(out["value"] - users * 1e3 / out["ms_per_step"]) <= 1e-6 * out["value"]
    assert not [k for k in FULL_ONLY if k in out]
    assert "score_parity_max_abs" not in out["config"]
    assert "secondary legs" not in r.stderr and "cpu baseline" not in r.stderr
    loss_sum = np.load(dump / "loss_sum.npy")
    scores = np.load(dump / "scores.npy")
    assert scores.shape == (users, 5) and np.isfinite(scores).all()
    assert np.isfinite(loss_sum) and abs(float(loss_sum) / users - out["loss"]) <= 1e-6 * abs(out["loss"])
    assert (dump / "param.news_encoder.word_embedding.0.weight.sampled_rows.npy").exists()
