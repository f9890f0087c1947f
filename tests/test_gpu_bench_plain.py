"""A plain bench.py run (no --full) at a small batch: it times exactly --steps steps, prints one
result line without the --full legs, and --dump-outputs writes what the last timed step returned."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_plain_run_dumps_outputs(tmp_path):
    B, out = 8, tmp_path / "dump"
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--batch", str(B), "--dump-outputs", str(out)]
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["full"] is False
    assert d["unit"] == "pairs/s" and d["higher_is_better"] is True and d["dtype"] == "bf16"
    # value and ms_per_step describe the same timed region (both rounded in the line)
    assert d["ms_per_step"] > 0 and abs(d["value"] * d["ms_per_step"] / 1000 / B - 1) < 1e-2
    assert d["roofline"] is None and d["cpu_baseline"] is None and "every_row" not in d
    assert "per-kernel" not in r.stderr

    got = {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}
    assert sorted(got) == ["image_features", "logits_per_image", "logits_per_text", "text_features"]
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in got.values())
    fi, ft = got["image_features"], got["text_features"]
    assert fi.shape == ft.shape == (B, 768) and got["logits_per_image"].shape == (B, B)
    np.testing.assert_allclose(np.linalg.norm(fi, axis=1), 1.0, rtol=1e-3)
    np.testing.assert_allclose(np.linalg.norm(ft, axis=1), 1.0, rtol=1e-3)
    # the logits are the f32 product of the dumped features at the model's initial scale 1 / 0.07; two f32
    # sums of 768 terms of unit vectors differ by at most 2 x 768 x 2^-24 x 14.3 = 1.3e-3
    np.testing.assert_allclose(got["logits_per_image"], fi @ ft.T / 0.07, atol=2e-3)
    assert np.array_equal(got["logits_per_text"], got["logits_per_image"].T)
