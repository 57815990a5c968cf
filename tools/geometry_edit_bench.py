#!/usr/bin/env python3
"""What a geometry edit costs, measured end to end on the host clock (bench.py measures the static frame only).

    python tools/geometry_edit_bench.py [--rounds R] [--edits K] [--out profiles/geometry_edit_bench.json]
                                        [--parent LIB]     an older build of libforma_hip.so as baseline (FORMA_HIP_LIB)

On `paris-like-30k-4k`, after warm-up, every variant measures
  (a) one replaced path: K times `clear` + `insert` of a 40-point path on one layer, then a device-resident frame; the clock runs
      from before the edit until the frame is complete (sync);
  (b) one inserted layer: a new layer per frame, removed again ten frames later (the removed layers' lines are garbage until
      compact_geom collects them: with 40-point paths on a 1.6 M-line scene that threshold — half the store — is never met, so
      the walk ends by removing the upper 55 % of the scene's layers, which makes compaction fire: the retain frame(s) are
      reported separately);
  (c) the static frame, for reference.
Variants: `resident` (Renderer(resident_geometry=True)), `default` (today's whole-scene upload) and, with --parent, `parent`
(the default path on the older library, the only path it has).  Boxes of a pool differ by 10-25 %, so the variants alternate
inside ONE run, each in a child process of its own (one build of the library per process), R rounds."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WORKLOAD = "paris-like-30k-4k"
CLEAR = (1.0, 1.0, 1.0, 1.0)


def summary(ms):
    ms = sorted(ms)
    if not ms:
        return None
    q = lambda f: ms[min(len(ms) - 1, int(f * len(ms)))]
    return {"n": len(ms), "median_ms": round(statistics.median(ms), 4), "p10_ms": round(q(0.10), 4), "p90_ms": round(q(0.90), 4),
            "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4)}


def polygon(api, cx, cy, rad, k=39):
    pb = api.PathBuilder().move_to(api.Point(cx + rad, cy))
    for j in range(1, k):
        pb.line_to(api.Point(float(np.float32(cx + rad * np.cos(2 * np.pi * j / k))), float(np.float32(cy + rad * np.sin(2 * np.pi * j / k)))))
    return pb.build()                                         # 39 vertices, closed: 40 points


def child(args):
    import gc
    from forma_amd import _lib, api, scenes
    fn, W, H = scenes.WORKLOADS[WORKLOAD]
    has_store = hasattr(_lib.lib(), "forma_hip_geometry_append")
    resident = args.mode == "resident" and has_store          # (an older library: the only path there is)
    comp = fn()
    n_layers = len(comp.layers)
    r = api.Renderer(0, resident_geometry=resident)
    ctx = r._ctx
    props = api.Props(func=api.Func.Draw(api.Style(fill=api.Fill.Solid(api.Color(0.2, 0.6, 0.3, 1.0)))))

    # where the host's part of an edit goes: compact_geom (the reference's garbage check, renderer.rs:113), the geometry store
    # (append / retain, or the whole-scene flatten and upload) and the layer / style tables, which are rebuilt as a whole
    spent = {"compact_geom": 0.0, "geometry": 0.0, "tables": 0.0}

    def timed(obj, name, key):
        fn = getattr(obj, name)

        def wrapper(*a, **k):
            t = time.perf_counter()
            try:
                return fn(*a, **k)
            finally:
                spent[key] += (time.perf_counter() - t) * 1e3
        setattr(obj, name, wrapper)
    timed(comp, "compact_geom", "compact_geom")
    timed(r, "_reconcile_geometry" if resident else "_upload_geometry", "geometry")
    timed(r, "_upload_tables", "tables")

    def frame():
        t0 = time.perf_counter()
        r._upload_scene(comp, None)
        t1 = time.perf_counter()
        ctx.render(W, H, clear=CLEAR, device_only=True)
        ctx.sync()
        return t0, t1, time.perf_counter()

    for _ in range(6):
        frame()
    # (c) the static frame of the whole scene, before anything is edited
    c_ms = []
    for _ in range(args.edits):
        t0 = time.perf_counter()
        ctx.render(W, H, clear=CLEAR, device_only=True)
        ctx.sync()
        c_ms.append((time.perf_counter() - t0) * 1e3)
    counters = (lambda: r.counters()) if has_store else (lambda: {})
    c0 = counters()
    # (a) one replaced path
    a_ms, a_scene_ms, a_frame_ms = [], [], []
    a_parts = {k: [] for k in spent}
    rng = np.random.default_rng(1)
    for i in range(args.edits):
        path = polygon(api, float(rng.uniform(200, W - 200)), float(rng.uniform(200, H - 200)), 60.0)
        for k in spent:
            spent[k] = 0.0
        t_edit = time.perf_counter()
        lay = comp.get_mut(api.Order(n_layers // 2))
        lay.clear(); lay.insert(path)
        _, t1, t2 = frame()
        a_ms.append((t2 - t_edit) * 1e3); a_scene_ms.append((t1 - t_edit) * 1e3); a_frame_ms.append((t2 - t1) * 1e3)
        for k in spent:
            a_parts[k].append(spent[k])
    c1 = counters()
    # (b) one inserted layer per frame, removed ten frames later; then the upper 55 % of the scene go and compaction fires
    b_ms, b_retain_ms = [], []
    live = []
    for i in range(args.edits):
        path = polygon(api, float(rng.uniform(200, W - 200)), float(rng.uniform(200, H - 200)), 60.0)
        before = len(comp._shared.pushes)
        t_edit = time.perf_counter()
        comp.get_mut_or_insert_default(api.Order(n_layers + i)).insert(path).set_props(props)
        live.append(n_layers + i)
        if len(live) > 10:
            gone = comp.remove(api.Order(live.pop(0))); del gone
        _, _, t2 = frame()
        (b_retain_ms if len(comp._shared.pushes) < before + 1 else b_ms).append((t2 - t_edit) * 1e3)
    for o in range(n_layers * 45 // 100, n_layers):
        gone = comp.remove(api.Order(o)); del gone
    gc.collect()
    t_removed = time.perf_counter()
    before = len(comp._shared.pushes)
    _, _, t2 = frame()
    if len(comp._shared.pushes) < before:
        b_retain_ms.append((t2 - t_removed) * 1e3)
    c2 = counters()
    out = {"mode": args.mode, "resident": resident, "library_has_store": has_store,
           "a_replace_path": summary(a_ms), "a_host_scene_part": summary(a_scene_ms), "a_frame_part": summary(a_frame_ms),
           "a_host_breakdown_median_ms": {k: round(statistics.median(v), 4) for k, v in a_parts.items()},
           "a_geometry_plus_frame": summary([g + f for g, f in zip(a_parts["geometry"], a_frame_ms)]), "b_insert_layer": summary(b_ms),
           "b_retain_frames": summary(b_retain_ms), "c_static": summary(c_ms),
           "counters_a": {k: c1[k] - c0[k] for k in c1 if k != "geometry_points"} if has_store else None,
           "counters_b": {k: c2[k] - c1[k] for k in c2 if k != "geometry_points"} if has_store else None}
    print(json.dumps(out))
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--edits", type=int, default=100)
    ap.add_argument("--parent", default=None, help="an older build of libforma_hip.so: the baseline variant")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "geometry_edit_bench.json"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--mode", default="resident")
    args = ap.parse_args()
    if args.child:
        return child(args)
    variants = ([("parent", args.parent)] if args.parent else []) + [("resident", None), ("default", None)]
    rounds = []
    for rd in range(args.rounds):
        row = {}
        for mode, lib in variants:
            env = dict(os.environ)
            if lib:
                env["FORMA_HIP_LIB"] = os.path.abspath(lib)
            else:
                env.pop("FORMA_HIP_LIB", None)
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--mode", mode, "--edits", str(args.edits)]
            p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
            line = [l for l in p.stdout.splitlines() if l.startswith("{")]
            if p.returncode != 0 or not line:
                print("%-9s FAILED (%d) %s" % (mode, p.returncode, (p.stderr or p.stdout)[-400:]), flush=True)
                return 1                                       # (nothing more is started on the device behind a failure)
            d = json.loads(line[-1])
            row[mode] = d
            print("round %d %-9s (a) %9.3f ms = %s + frame %.3f  (b) %9.3f ms  retain %s  (c) %7.3f ms" % (
                rd, mode, d["a_replace_path"]["median_ms"], d["a_host_breakdown_median_ms"], d["a_frame_part"]["median_ms"],
                d["b_insert_layer"]["median_ms"], d["b_retain_frames"] and d["b_retain_frames"]["median_ms"], d["c_static"]["median_ms"]), flush=True)
        rounds.append(row)
    result = {"workload": WORKLOAD, "edits": args.edits, "clock": "host, from before the edit until the device-resident frame is complete",
              "rounds": rounds}
    result["ratio_default_over_resident_a_geometry_plus_frame"] = [round(r["default"]["a_geometry_plus_frame"]["median_ms"] / r["resident"]["a_geometry_plus_frame"]["median_ms"], 1) for r in rounds]
    if args.parent:
        result["ratio_parent_over_resident_a_geometry_plus_frame"] = [round(r["parent"]["a_geometry_plus_frame"]["median_ms"] / r["resident"]["a_geometry_plus_frame"]["median_ms"], 1) for r in rounds]
        result["ratio_parent_over_resident_a"] = [round(r["parent"]["a_replace_path"]["median_ms"] / r["resident"]["a_replace_path"]["median_ms"], 1) for r in rounds]
        result["resident_below_parent_in_every_round"] = all(r["resident"]["a_replace_path"]["median_ms"] < r["parent"]["a_replace_path"]["median_ms"] for r in rounds)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("written:", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
