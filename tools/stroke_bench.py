#!/usr/bin/env python3
"""What stroking costs on the device, recorded (nothing is gated on it).

    python tools/stroke_bench.py [--rounds R] [--width W] [--out profiles/stroke_bench.json] [--no-kernels]

Every path of `paris-like-30k-4k` (1.6 M source points) is stroked with round joins and with bevel joins in ONE
forma_hip_geometry_append_stroked call on an empty store.  Reported per variant:
  * the whole call on the host clock (work items packed on the host, one upload, flatten, count + scan, the wait for the total,
    emit, the second wait), median of R rounds after a warm-up;
  * source points, output points, and the bytes the stroke kernels must read and write at the least: 12 B per source point into
    each of the count and emit passes, 4 B per source point of counts written and read back, 12 B per output point written;
  * from a second run of this script under `rocprofv3 --kernel-trace --stats` (the dispatches' own timestamps): the average time of
    k_stroke_count, k_stroke_scan, k_stroke_emit, and so the rate each achieved.
Yardsticks from the same run, same box: the same paths through forma_hip_geometry_append (k_flatten_store: 16 B in, 12 B out per
point) and forma_hip_geometry_retain of the whole stroked store (k_geom_retain: 24 B per surviving point, a pure streaming copy).
If the emit pass runs below half of k_geom_retain's rate the output says so."""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WORKLOAD = "paris-like-30k-4k"


def run(args):
    import forma_amd
    from forma_amd import api, scenes
    fn, _, _ = scenes.WORKLOADS[WORKLOAD]
    comp = fn()
    paths = [p for _, p, _ in comp._shared.pushes]
    H = api._host()
    ctx = forma_amd.Context(0)
    empty = lambda: ctx.set_geometry(np.zeros(0, np.float32), np.zeros(0, np.float32), np.zeros(0, np.uint32))
    out = {"workload": WORKLOAD, "paths": len(paths), "stroke_width": args.width, "rounds": args.rounds, "variants": {}}

    def batch_of(items):
        b = H.forma_host_batch_new()
        for k, p in enumerate(items):
            H.forma_host_batch_add(b, p._h, k)
        return b

    def timed_appends(items):
        b = batch_of(items)
        src = int(H.forma_host_batch_points(b))
        ms, added = [], C.c_size_t(0)
        for r in range(args.rounds + 1):
            empty()
            t0 = time.perf_counter()
            ctx._check(H.forma_host_batch_append_stroked(b, ctx._h, C.byref(added)))
            if r:                                                  # (round 0 grows the buffers)
                ms.append((time.perf_counter() - t0) * 1e3)
        H.forma_host_batch_free(b)
        return src, int(added.value), statistics.median(ms)

    src, n, ms = timed_appends(paths)
    out["variants"]["filled"] = {"source_points": src, "points": n, "call_ms": round(ms, 3),
                                 "kernel": "k_flatten_store", "kernel_bytes": 28 * src}
    for name, join in (("round", api.StrokeJoin.Round), ("bevel", api.StrokeJoin.Bevel)):
        st = api.StrokeStyle(args.width, join, api.StrokeCap.Butt)
        src, n, ms = timed_appends([p.stroke(st) for p in paths])
        v = {"source_points": src, "points": n, "call_ms": round(ms, 3),
             "bytes": {"k_stroke_count": 12 * src + 4 * src, "k_stroke_scan": 8 * ((src + 255) // 256), "k_stroke_emit": 12 * src + 4 * src + 12 * n}}
        # the yardstick on the same store: everything survives one retain (a streaming copy of the stroked store)
        ctx.n_points = n
        rms = []
        for r in range(args.rounds + 1):
            t0 = time.perf_counter()
            ctx.geometry_retain([(0, n)], np.arange(len(paths), dtype=np.uint32))
            if r:
                rms.append((time.perf_counter() - t0) * 1e3)
        v["retain_call_ms"] = round(statistics.median(rms), 3)
        v["retain_bytes"] = 24 * n
        out["variants"][name] = v
    ctx.close()
    return out


def kernel_times(args):
    """this script again, under the profiler: {kernel: [average ns per call, in call order of the variants]}"""
    d = tempfile.mkdtemp(prefix="stroke_bench_")
    cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), "--child",
           "--rounds", "2", "--width", str(args.width)]
    subprocess.run(cmd, check=True, capture_output=True, text=True, cwd=ROOT, timeout=args.child_timeout)
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    times = {}
    for r in rows:
        name = r["Kernel_Name"].split("(")[0].replace("void ", "").strip()
        if name.startswith(("k_stroke_", "k_flatten_store", "k_geom_retain")):
            times.setdefault(name, []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--width", type=float, default=2.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stroke_bench.json"))
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--child-timeout", type=int, default=300)
    args = ap.parse_args()
    out = run(args)
    if args.child:
        return
    if not args.no_kernels:
        # dispatches in launch order: filled (rounds + 1 calls), then per stroked variant rounds + 1 appends and rounds + 1 retains
        t = kernel_times(args)
        k = 3                                                       # the child's calls per variant (--rounds 2)
        med = lambda v: float(statistics.median(v)) / 1e3
        us = {"filled": {"k_flatten_store": med(t["k_flatten_store"][1:k])}}
        for i, name in enumerate(("round", "bevel")):
            sl = slice(i * k + 1, (i + 1) * k)
            us[name] = {kn: med(t[kn][sl]) for kn in ("k_stroke_count", "k_stroke_scan", "k_stroke_emit", "k_geom_retain")}
            us[name]["k_flatten_store"] = med(t["k_flatten_store"][k + i * k + 1: k + (i + 1) * k])
        out["variants"]["filled"]["kernel_us"] = round(us["filled"]["k_flatten_store"], 2)
        out["variants"]["filled"]["kernel_GBps"] = round(out["variants"]["filled"]["kernel_bytes"] / us["filled"]["k_flatten_store"] / 1e3, 1)
        for name in ("round", "bevel"):
            v = out["variants"][name]
            v["kernel_us"] = {kn: round(x, 2) for kn, x in us[name].items()}
            v["GBps"] = {kn: round(v["bytes"][kn] / us[name][kn] / 1e3, 1) for kn in ("k_stroke_count", "k_stroke_emit")}
            v["GBps"]["k_geom_retain"] = round(v["retain_bytes"] / us[name]["k_geom_retain"] / 1e3, 1)
            v["emit_vs_retain_rate"] = round(v["GBps"]["k_stroke_emit"] / v["GBps"]["k_geom_retain"], 3)
            if v["emit_vs_retain_rate"] < 0.5:
                v["note"] = ("the emit pass runs below half of k_geom_retain's streaming rate: a lane writes its own run of 4 to 12 "
                             "consecutive points, 4 B at a time per array, so a wavefront's store touches 64 separate runs instead of one "
                             "contiguous 256 B row, and every lane first walks its neighbours and divides and takes a square root per line")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
