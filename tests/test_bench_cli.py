"""bench.py's command line: a plain run is the headline measurement alone, --full adds the other
legs, --dump-outputs writes the last timed step's arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("roofline", "fused_sine_gemm", "psnr", "configs", "cpu_baseline", "cpu_baselines")


def test_parse_plain_and_full(monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--no-psnr", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.no_psnr and not a.no_cpu_baseline and a.dump_outputs == "d"
    assert (a.steps, a.warmup) == bench.CONFIG_DEFAULT_STEPS["m"]


@pytest.mark.gpu
def test_plain_run_dumps_outputs(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["higher_is_better"] is True
    assert abs(d["value"] - d["config"]["global_batch"] / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    assert not [k for k in FULL_ONLY if k in d]
    files = sorted(os.listdir(tmp_path / "out"))
    assert "loss.npy" in files and "model_out.npy" in files and "param_000.npy" in files
    arrays = {f: np.load(tmp_path / "out" / f, allow_pickle=False) for f in files}
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in arrays.values())
    assert arrays["model_out.npy"].shape == (1, 512 * 512, 1)
    assert sum(os.path.getsize(tmp_path / "out" / f) for f in files) <= 64 << 20
