"""bench.py without --full: the headline line alone (no side legs), exactly --steps timed steps, and --dump-outputs writing the
same samples of the last step's frames in two runs with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(out_dir):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--frames-per-gpu", "2", "--dump-outputs", out_dir], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_plain_run_prints_the_headline_and_dumps_the_same_outputs_twice(tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    line = run_bench(a)
    assert line["unit"] == "Mpixels/s" and line["higher_is_better"] is True and line["dtype"] == "f32" and line["metric"]
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
    # value and ms_per_step describe the same timed steps: 2 frames of 3840 x 2160 per step
    assert abs(line["value"] - 2 * 3840 * 2160 / (line["ms_per_step"] * 1e3)) < 0.01 * line["value"]
    assert not {"also", "cpu_baseline", "roofline", "untimed", "gather", "timing"} & set(line)
    files = sorted(os.listdir(a))
    assert files == ["frame0.npy", "frame1.npy"]
    assert sum(os.path.getsize(os.path.join(a, f)) for f in files) <= 64e6
    run_bench(b)
    for f in files:
        x, y = np.load(os.path.join(a, f)), np.load(os.path.join(b, f))
        assert x.dtype == np.float32 and x.size > 1000000 and np.array_equal(x.view(np.uint32), y.view(np.uint32)), f
