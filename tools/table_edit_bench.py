#!/usr/bin/env python3
"""What moving the layers costs: frames/s of a scene whose layer table changes before EVERY frame (bench.py measures the static
frame only).

    python tools/table_edit_bench.py [--frames K] [--repeats R] [--renderer-frames F] [--out profiles/table_edit_bench.json]

On `paris-like-30k-4k`, device-resident frames, with one and with three frame slots, after warm-up:
  motions  pan        the reference demo's pan: the same translate on every layer, a few pixels per frame
           zoom       1 % per frame about the canvas centre (25 frames out, then back to 1)
           one_layer  one layer moves, the others stay
  routes   set_geoms  forma_hip_set_geoms with the whole table before every frame (the code of the parent commit: the yardstick)
           entries    forma_hip_update_geoms (pan / zoom: every slot; one_layer: that slot)
           xf         forma_hip_update_geoms_xf (pan / zoom: the whole range; one_layer: a range of one)
  static   no edit at all, for reference
Every cell is a fresh context; the tables of the frames are built before the clock starts, so a cell times the scene call and
the frame, not numpy.  Per cell: frames/s over K frames (the clock stops after forma_hip_sync), the host time inside the scene
call (median), and the counters' growth: frames_rerun, frames_learned, scene_drains, table_edit_bytes_h2d.
The routes alternate inside one process and the whole list is repeated R times (processes of their own, one after the other):
the difference between two repeats of the set_geoms route is the spread the other routes are judged against.
Then the same pan through `api.Renderer`, default against `resident_tables=True` (F frames, three frame slots): there the
Python side — 30 000 `set_transform` calls and, on the default path, the rebuild of all tables — is part of the frame.
Nothing more is started on the device behind a child that failed."""
import argparse
import json
import os
import statistics
import subprocess
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WORKLOAD = "paris-like-30k-4k"
CLEAR = (1.0, 1.0, 1.0, 1.0)
PERIOD = 25
MOTIONS = ("pan", "zoom", "one_layer")
ROUTES = ("set_geoms", "entries", "xf")


def motion_xf(motion, k, W, H):
    j = k % PERIOD
    if motion == "zoom":
        s = float(np.float32(1.01 ** j))
        return (s, 0.0, 0.0, s, float(np.float32(W / 2 * (1 - s))), float(np.float32(H / 2 * (1 - s))))
    return (1.0, 0.0, 0.0, 1.0, 3.0 * (j + 1), 2.0 * (j + 1))


def cell(forma_amd, t, W, H, slots, motion, route, frames):
    c = forma_amd.Context(0, frames_in_flight=slots)
    c.set_geometry(t["x"], t["y"], t["line_slot"]); c.set_geoms(t["geoms"])
    c.set_styles(t["style_offsets"], t["style_words"], None); c.set_images(t["images"], t["texels"])
    base = np.array(t["geoms"])
    n = len(base)
    one = n // 2
    while base["order"][one] == 0xFFFFFFFF:
        one += 1
    lo, cnt = (one, 1) if motion == "one_layer" else (0, n)
    xfs = [motion_xf(motion, k, W, H) for k in range(PERIOD)]
    tables = None
    if route != "xf" and motion != "static":
        tables = []
        for xf in xfs:
            g = base.copy()
            g["flags"][lo:lo + cnt] = 1; g["xf"][lo:lo + cnt] = xf
            tables.append(g if route == "set_geoms" else np.ascontiguousarray(g[lo:lo + cnt]))
    all_slots = np.arange(lo, lo + cnt, dtype=np.uint32)
    xfa = [np.array(xf, np.float32) for xf in xfs]

    def edit(k):
        j = k % PERIOD
        if route == "set_geoms":
            c.set_geoms(tables[j])
        elif route == "entries":
            c.update_geoms(all_slots, tables[j])
        else:
            c.update_geoms_xf(lo, cnt, xfa[j])

    for k in range(3 * slots + 3 + PERIOD):                   # every slot learns; then one period of the motion, so that its largest frame has been seen
        if motion != "static":
            edit(k)
        c.render(W, H, clear=CLEAR, device_only=True)
    c.sync()
    c0 = c.counters()
    call_us = []
    t0 = time.perf_counter()
    for k in range(frames):
        if motion != "static":
            ta = time.perf_counter()
            edit(k)
            call_us.append((time.perf_counter() - ta) * 1e6)
        c.render(W, H, clear=CLEAR, device_only=True)
    c.sync()
    dt = time.perf_counter() - t0
    c1 = c.counters()
    img = c.read_image(W, H)
    c.close()
    grow = lambda k: int(c1.get(k, 0) - c0.get(k, 0))
    return {"fps": round(frames / dt, 1), "scene_call_us_median": round(statistics.median(call_us), 2) if call_us else 0.0,
            "scene_call_us_p90": round(sorted(call_us)[int(0.9 * len(call_us))], 2) if call_us else 0.0,
            "frames_rerun": grow("frames_rerun"), "frames_learned": grow("frames_learned"), "scene_drains": grow("scene_drains"),
            "table_edits": grow("table_edits"), "table_edit_bytes_h2d": grow("table_edit_bytes_h2d"),
            "crc": int(np.bitwise_xor.reduce(img.view(np.uint32).reshape(-1))) & 0xFFFFFFFF}


def child_abi(args):
    import forma_amd
    from forma_amd import scenes
    t = np.load(args.scene)
    _, W, H = scenes.WORKLOADS[WORKLOAD]
    out = {}
    for slots in (1, 3):
        row = {"static": cell(forma_amd, t, W, H, slots, "static", "none", args.frames)}
        for motion in MOTIONS:
            for route in ROUTES:                                  # the routes alternate: set_geoms, entries, xf, set_geoms, ...
                row[motion + "/" + route] = cell(forma_amd, t, W, H, slots, motion, route, args.frames)
        out["slots_%d" % slots] = row
    print(json.dumps(out))


def child_renderer(args):
    from forma_amd import api, scenes
    fn, W, H = scenes.WORKLOADS[WORKLOAD]
    comp = fn()
    out = {}
    for name, resident in (("default", False), ("resident_tables", True), ("default_again", False)):
        r = api.Renderer(0, frames_in_flight=3, resident_tables=resident)
        ctx = r._ctx

        def frame(k):
            xf = api.GeomPresTransform.try_from(list(motion_xf("pan", k, W, H)))
            for layer in comp.layers.values():
                layer.set_transform(xf)
            t0 = time.perf_counter()
            r._upload_scene(comp, None)
            t1 = time.perf_counter()
            ctx.render(W, H, clear=CLEAR, device_only=True)
            return (t1 - t0) * 1e3
        for k in range(12):
            frame(k)
        ctx.sync()
        c0 = r.counters()
        t0 = time.perf_counter()
        scene_ms = [frame(k) for k in range(args.renderer_frames)]
        ctx.sync()
        dt = time.perf_counter() - t0
        c1 = r.counters()
        out[name] = {"fps": round(args.renderer_frames / dt, 2), "upload_scene_ms_median": round(statistics.median(scene_ms), 3),
                     "scene_drains": c1["scene_drains"] - c0["scene_drains"], "table_edits": c1["table_edits"] - c0["table_edits"],
                     "frames_rerun": c1["frames_rerun"] - c0["frames_rerun"], "frames_learned": c1["frames_learned"] - c0["frames_learned"]}
        ctx.close()
    print(json.dumps(out))


def run_child(what, args):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", what, "--frames", str(args.frames), "--renderer-frames", str(args.renderer_frames), "--scene", args.scene]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.child_timeout)
    line = [l for l in p.stdout.splitlines() if l.startswith("{")]
    if p.returncode != 0 or not line:
        print("%s FAILED (%d) %s" % (what, p.returncode, (p.stderr or p.stdout)[-600:]), flush=True)
        return None
    return json.loads(line[-1])


def judge(repeats):
    """per frame-slot count and motion: the spread of the yardstick (set_geoms, two repeats) and each edit route against it"""
    verdict = {}
    for slots in ("slots_1", "slots_3"):
        static = [r[slots]["static"]["fps"] for r in repeats]
        v = {"static_fps": static}
        for motion in MOTIONS:
            base = [r[slots][motion + "/set_geoms"]["fps"] for r in repeats]
            spread = max(base) - min(base)
            m = {"set_geoms_fps": base, "spread_fps": round(spread, 1)}
            for route in ("entries", "xf"):
                fps = [r[slots][motion + "/" + route]["fps"] for r in repeats]
                m[route + "_fps"] = fps
                m[route + "_gain_over_set_geoms_fps"] = round(min(fps) - max(base), 1)       # the worst repeat against the yardstick's best
                m[route + "_beats_set_geoms_by_more_than_the_spread"] = bool(min(fps) - max(base) > spread)
                m[route + "_not_slower_beyond_the_spread"] = bool(min(fps) >= min(base) - spread)
                m[route + "_below_static"] = "%.1f %%" % (100.0 * (1.0 - statistics.median(fps) / statistics.median(static)))
            v[motion] = m
        verdict[slots] = v
    return verdict


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--renderer-frames", type=int, default=40)
    ap.add_argument("--child-timeout", type=int, default=420)
    ap.add_argument("--no-renderer", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "table_edit_bench.json"))
    ap.add_argument("--child", default=None)
    ap.add_argument("--scene", default=None, help="(children) the scene's flat tables, written by the parent into a directory of this run")
    args = ap.parse_args()
    if args.child == "abi":
        return child_abi(args)
    if args.child == "renderer":
        return child_renderer(args)
    workdir = tempfile.mkdtemp(prefix="table_edit_bench_")   # the scene's flat tables, built by THIS run and removed with it
    try:
        return measure(args, workdir)
    finally:
        shutil.rmtree(workdir, ignore_errors=True)


def measure(args, workdir):
    from forma_amd import api, scenes
    fn, W, H = scenes.WORKLOADS[WORKLOAD]
    r = api.Renderer(0)
    r.render(fn(), api.BufferBuilder(np.zeros(W * H * 4, np.uint8), api.LinearLayout(W, W * 4, H)).build(), api.RGBA, api.Color(1, 1, 1, 1), None)
    args.scene = os.path.join(workdir, "scene.npz")
    np.savez(args.scene, **r.host_tables)
    r._ctx.close()
    repeats = []
    for rep in range(args.repeats):
        d = run_child("abi", args)
        if d is None:
            return 1
        repeats.append(d)
        for slots, row in d.items():
            for name, c in row.items():
                print("repeat %d %-8s %-20s %8.1f frames/s  call %8.2f us  rerun %3d learned %3d drains %3d  h2d %9d B" % (
                    rep, slots, name, c["fps"], c["scene_call_us_median"], c["frames_rerun"], c["frames_learned"], c["scene_drains"], c["table_edit_bytes_h2d"]), flush=True)
    result = {"workload": WORKLOAD, "frames": args.frames, "period": PERIOD,
              "clock": "host, K frames with the scene call in front of each, until forma_hip_sync returns; device-resident frames",
              "repeats": repeats, "verdict": judge(repeats)}
    crcs = {(m, r[s][m + "/" + rt]["crc"]) for r in repeats for s in r for m in MOTIONS for rt in ROUTES}
    result["last_images_identical_across_routes_and_slots"] = len(crcs) == len(MOTIONS)
    if not args.no_renderer:
        d = run_child("renderer", args)
        if d is None:
            result["renderer_pan"] = "not measured: the child failed"
        else:
            result["renderer_pan"] = d
            print("api.Renderer pan:", d, flush=True)
    else:
        result["renderer_pan"] = "not measured"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result["verdict"], indent=1))
    print("written:", args.out)
    if not result["last_images_identical_across_routes_and_slots"]:
        print("FAILED: the routes' last images differ (same motion, same frame number: they must be identical)")
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
