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


def test_bench_plain_run_is_the_headline_and_full_adds_the_other_legs(tmp_path):
    base = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1", "--workload", "cubics-1080p"]
    extra = ("fps_blocks", "fps_render_call", "fps_including_d2h", "stages_us", "kernels_us", "roofline", "roofline_painter",
             "animated", "cpu_baseline")
    lines = {}
    for name, flags in (("plain", []), ("full", ["--full", "--no-animated", "--no-cpu-baseline", "--no-pmc", "--no-d2h"])):
        p = subprocess.run(base + flags, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
        assert p.returncode == 0, p.stderr[-2000:]
        lines[name] = json.loads(p.stdout.strip().splitlines()[-1])
    for line in lines.values():
        assert line["steps"] == 4 and line["warmup"] == 1 and line["value"] > 0 and line["ms_per_step"] > 0
        assert line["unit"] == "frames/s" and line["higher_is_better"] is True and line["config"]["canvas"] == [1920, 1080]
    assert lines["plain"]["full"] is False and not any(k in lines["plain"] for k in extra)
    full = lines["full"]
    assert full["full"] is True and full["fps_blocks"]["blocks"] == 5 and full["fps_render_call"]["median"] > 0
    assert full["stages_us"]["total_us"] > 0 and full["kernels_us"]
    assert full["roofline"]["passes"] > 0 and "animated" not in full and "cpu_baseline" not in full
