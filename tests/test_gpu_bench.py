"""A plain `bench.py --gpus 1` run: the headline and nothing else.  Set-up, warm-up, the timed regions, --dump-outputs and the one JSON
line; the roofline pass, the secondary legs and the CPU baseline run only with --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_is_the_headline_only(tmp_path):
    steps, warmup = 4, 1
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                        "--preheat-ms", "0", "--dump-outputs", str(tmp_path)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    assert d["metric"] == "signal samples/s basecalled (chunk=1024, beam=10)" and d["unit"] == "samples/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f32" and d["n_gpus"] == 1 and d["steps"] == steps and d["warmup"] == warmup
    assert d["value"] > 0 and abs(d["value"] - steps * 64 * 4096 / (d["ms_per_step"] * 1e-3 * steps)) <= 1e-6 * d["value"]
    assert len(d["value_runs"]) == 3 and min(d["value_runs"]) <= d["value"] <= max(d["value_runs"])
    # what moved behind --full
    assert d["roofline"] is None and "cpu_baseline" not in d and "gpu_over_cpu" not in d
    assert not [k for k in d if k.startswith("secondary")], sorted(d)
    # the last timed step's labels, as before
    lab = np.load(tmp_path / "labels.npy")
    ln = np.load(tmp_path / "label_lengths.npy")
    assert lab.shape == (512, 1024) and lab.dtype == np.float32 and ln.shape == (512,) and ln.dtype == np.float32
    assert ln.min() >= 0 and ln.max() <= 1024 and ln.sum() > 0
    inside = np.arange(1024)[None, :] < ln[:, None]
    assert np.all(lab[~inside] == -1.0) and np.all((lab[inside] >= 0) & (lab[inside] <= 3))
