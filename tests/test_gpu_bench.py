"""bench.py end to end on the GPU: `--steps` sets the timed steps, the line carries `ms_per_step`, and `--dump-outputs` writes
the image of the timed path — equal to what the public API renders for the same seeded workload."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_dump_outputs_hold_the_image_the_api_renders(tmp_path):
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1", "--workload", "cubics-1080p",
           "--no-animated", "--no-cpu-baseline", "--no-pmc", "--no-d2h", "--dump-outputs", str(out)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert line["steps"] == 4 and line["ms_per_step"] > 0
    assert line["dump_outputs"]["files"] == {"image_row_sums.npy": [1080, 4], "image_rgba.npy": [1080, 1920, 4]}

    from forma_amd import api, scenes
    img = np.zeros((1080, 1920 * 4), np.uint8)
    r = api.Renderer()
    r.render(scenes.random_cubics(), api.BufferBuilder(img.reshape(-1), api.LinearLayout(1920, 1920 * 4, 1080)).build(), api.RGBA,
             api.Color(1.0, 1.0, 1.0, 1.0), None)
    r._ctx.close()
    want = img.reshape(1080, 1920, 4)
    assert (want != 255).any()
    got = np.load(out / "image_rgba.npy")
    assert got.dtype == np.float32 and np.array_equal(got, want.astype(np.float32))
    assert np.array_equal(np.load(out / "image_row_sums.npy"), want.sum(axis=1, dtype=np.float64))
