"""bench.py without --full: set-up, warm-up, the timed steps, --dump-outputs and the result line -- nothing that takes runs of its own."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent


def test_plain_bench_measures_the_headline_alone(tmp_path):
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--dump-outputs", str(out)],
                       cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout[-4000:]
    d = json.loads(lines[0])
    assert d["metric"] == "512x512 tiles/sec fwd+bwd (4-ch->5-class U-Net)" and d["unit"] == "tiles/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f32" and d["steps"] == 2 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["value"] > 0 and d["ms_per_step"] > 0 and abs(d["value"] - 16 * 1e3 / d["ms_per_step"]) < 1e-2 * d["value"]
    assert np.isfinite(d["loss"]) and d["roofline"]["launches_per_step"] > 0
    assert "secondary" not in d and "cpu_baseline" not in d
    assert "secondary:" not in r.stderr and "cpu_baseline" not in r.stderr
    for name in ("loss", "logits", "params", "grads", "buffers"):
        a = np.load(out / f"{name}.npy")
        assert a.size > 0 and np.isfinite(a).all(), name
