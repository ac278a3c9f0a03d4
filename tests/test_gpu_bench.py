"""A plain `bench.py` run on the device, at a small batch: one JSON line with the headline fields and none of the --full legs,
and --dump-outputs writing the sampled windows."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_bench_line_is_the_headline(tmp_path):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--batch", "64", "--unique", "2", "--steps", "2", "--warmup", "1",
                          "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    r = json.loads(lines[0])
    assert r["unit"] == "solves/s" and r["higher_is_better"] is True and r["dtype"] == "f64"
    assert r["value"] > 0 and abs(r["ms_per_step"] - 1e3 * 64 / r["value"]) < 1e-6 * r["ms_per_step"]
    for leg in ("roofline", "cpu_baseline", "end_to_end", "mixed_batch", "resident_1024", "single_window", "other_configs"):
        assert leg not in r, leg
    cost = np.load(tmp_path / "summary_final_cost.npy")
    assert cost.shape == (64,) and np.all(np.isfinite(cost))
