"""Where does the fused first digit pass (csrc/sort.hip, SliceSrc) stop paying?  A/B of FORMA_HIP_DEBUG=fuse_digit=0 against
fuse_digit=2 over scenes whose (digit, block) slices range from a few keys to hundreds: many small triangles scattered over a 4K
canvas in paint order (a 2 048-segment block then touches many tile columns: short slices), larger ones, and the headline
stand-in.  Per scene and switch: the median of rasterize_us + sort_us over timed read-back-free frames, and the mean slice
length (segments / distinct (block, first digit) pairs of the unsorted stream; the first digit of these layer-sorted 4K plans
is tile_x + 1).  FUSE_MIN_SLICE in csrc/api.cpp is set from the break-even this prints.

    python tools/fuse_sweep.py [--frames 30] [--out sweep.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from forma_amd import api, scenes  # noqa: E402

W, H = 3840, 2160
CLEAR = (1.0, 1.0, 1.0, 1.0)


def scattered(n, size, seed=1):
    comp = api.Composition()
    rng = np.random.default_rng(seed)
    for i in range(n):
        x, y = float(rng.uniform(0, W - size)), float(rng.uniform(0, H - size))
        comp.get_mut_or_insert_default(i).insert(
            api.PathBuilder().move_to(api.Point(x, y)).line_to(api.Point(x + size, y + size / 3))
            .line_to(api.Point(x + size / 2, y + size)).build()).set_props(scenes._solid(api.Color(0.3, 0.5, (i % 5) / 5.0, 0.8)))
    return comp


def run(comp, switch, frames):
    os.environ["FORMA_HIP_DEBUG"] = switch
    image = np.zeros((H, W * 4), np.uint8)
    r = api.Renderer(device=0)
    try:
        r.render(comp, api.BufferBuilder(image.reshape(-1), api.LinearLayout(W, W * 4, H)).build(), api.RGBA, api.Color(*CLEAR), None)
        ctx = r._ctx
        for _ in range(3):
            ctx.render(W, H, clear=CLEAR)
        t, fused, tm = [], False, None
        for _ in range(frames):
            _img, tm = ctx.render(W, H, clear=CLEAR, timings=True)
            t.append(tm["rasterize_us"] + tm["sort_us"])
            fused = "k_slice_scan" in [k[0] for k in ctx.kernel_times()]
        seg = ctx.segments(0)
        blk = np.arange(len(seg), dtype=np.int64) // 2048
        d0 = (seg >> np.uint64(41)).astype(np.int64) & 0xFFF
        slices = len(np.unique(blk * 4096 + d0))
        return {"us": float(np.median(t)), "fused": fused, "n": int(tm["n_segments"]), "passes": int(tm["n_sort_passes"]),
                "mean_slice": len(seg) / max(slices, 1)}
    finally:
        r._ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cases = [("scattered-%d-%gpx" % (n, s), lambda n=n, s=s: scattered(n, s)) for n, s in
             ((150000, 3), (100000, 6), (60000, 10), (40000, 20), (20000, 40), (8000, 80), (4000, 160))]
    cases.append(("paris-like-30k-4k", lambda: scenes.paris_like()))
    rows = []
    for name, build in cases:
        comp = build()
        off = run(comp, "fuse_digit=0", a.frames)
        on = run(comp, "fuse_digit=2", a.frames)
        row = {"scene": name, "n": off["n"], "passes": off["passes"], "mean_slice": round(on["mean_slice"], 1),
               "fused_ran": on["fused"], "plain_us": round(off["us"], 1), "fused_us": round(on["us"], 1),
               "gain_us": round(off["us"] - on["us"], 1)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
