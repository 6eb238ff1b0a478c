"""bench.py as the benchmark driver runs it: a plain run (no --full) prints the one JSON line of the headline and, with
--dump-outputs, what its last timed step returned."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_line_and_dumped_outputs(tmp_path):
    steps, batch, size = 3, 2, 256
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [
        os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--batch", str(batch), "--size", str(size),
        "--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line, key
    assert line["steps"] == steps and line["unit"] == "images/sec" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["ms_per_step"] > 0 and abs(line["value"] - batch / (line["ms_per_step"] * 1e-3)) <= 0.01 * line["value"]
    for extra in ("kernel_families", "fast_mode", "nms_micro", "postproc", "train_step", "cpu_baseline"):     # --full only
        assert extra not in line, extra
    d = {n: np.load(tmp_path / "out" / f"{n}.npy") for n in ("scores", "classes", "boxes", "counts")}
    assert all(a.dtype == np.float32 for a in d.values())
    assert d["scores"].shape == (batch, 1000) and d["classes"].shape == (batch, 1000) and d["boxes"].shape == (batch, 1000, 4)
    assert d["counts"].tolist() == line["detections_kept_rank0"][:batch]
    for b, n in enumerate(d["counts"].astype(int)):
        assert np.all(d["scores"][b, :n] >= 0.05) and np.all(d["scores"][b, n:] == 0)
        assert np.all((d["classes"][b, :n] >= 1) & (d["classes"][b, :n] <= 80))
        assert np.all((d["boxes"][b, :n] >= 0) & (d["boxes"][b, :n] <= size - 1))
