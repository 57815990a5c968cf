#!/usr/bin/env python3
"""frames/s of one context by where the frame lands: caller host memory (a registered buffer; three of them through
forma_hip_render_enqueue with frame slots), the context's own image (dst == NULL), and caller device memory through
forma_hip_render_device as SRGB8 and as LINEAR_F16 (torch tensors; four in turn with frame slots).  Every leg with 1 and 3 frame
slots, and the painter's kernel time per frame (forma_hip_kernel_times, stage 4) for u8 against f16.

    python tools/device_target_bench.py [--workloads paris-like-30k-4k,cubics-1080p] [--out profiles/device_target_bench.json]

Each workload runs in a child process of its own under `timeout -k 10`; the parent touches no GPU."""
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
CLEAR = (1.0, 1.0, 1.0, 1.0)


def child(wl, frames, runs):
    import torch                                                    # (first: one HIP runtime for torch and the library)
    from forma_amd import api, scenes
    build, W, H = scenes.WORKLOADS[wl]
    comp = build()
    dev = torch.device("cuda", 0)
    r = api.Renderer(0)
    img = np.zeros((H, W * 4), np.uint8)
    r.render(comp, api.BufferBuilder(img.reshape(-1), api.LinearLayout(W, W * 4, H)).build(), api.RGBA, api.Color(*CLEAR), None)
    ctx = r._ctx
    stream = torch.cuda.current_stream(dev).cuda_stream
    hosts = [np.zeros((H, W * 4), np.uint8) for _ in range(3)]
    for b in hosts:
        ctx.register_buffer(b)
    tens = {"srgb8": [torch.zeros((H, W, 4), dtype=torch.uint8, device=dev) for _ in range(4)],
            "linear_f16": [torch.zeros((H, W, 4), dtype=torch.float16, device=dev) for _ in range(4)]}
    k = [0]

    def leg(name, slots):
        if name == "host_dst":
            if slots == 1:
                return lambda: ctx.render(W, H, clear=CLEAR, dst=hosts[0])
            return lambda: ctx.render_enqueue(W, H, hosts[k[0] % 3], clear=CLEAR)
        if name == "dst_null":
            return lambda: ctx.render(W, H, clear=CLEAR, device_only=True)
        t = tens[name.replace("device_", "")]
        fmt = name.replace("device_", "")
        return lambda: ctx.render_device(t[k[0] % 4].data_ptr(), fmt, W, H, t[0].stride(0) * t[0].element_size(), clear=CLEAR,
                                         wait_stream=stream)

    out = {"workload": wl, "width": W, "height": H, "frames_per_run": frames, "runs": runs, "fps": {}}
    for slots in (1, 3):
        ctx.set_frames_in_flight(slots)
        for name in ("host_dst", "dst_null", "device_srgb8", "device_linear_f16"):
            fn = leg(name, slots)

            def step():
                fn(); k[0] += 1
            for _ in range(10):
                step()
            ctx.sync(); torch.cuda.synchronize()
            rates = []
            for _ in range(runs):
                t0 = time.perf_counter()
                for _ in range(frames):
                    step()
                ctx.sync()
                rates.append(frames / (time.perf_counter() - t0))
            out["fps"][f"{name}/slots={slots}"] = {"median": round(statistics.median(rates), 1), "all": [round(x, 1) for x in rates]}
    ctx.set_frames_in_flight(1)
    # the painter's device time per frame (stage 4 of forma_hip_kernel_times: k_paint_* launches), u8 vs f16 target
    paint = {}
    for fmt in ("srgb8", "linear_f16"):
        t = tens[fmt][0]
        per = []
        for i in range(25):
            ctx.render_device(t.data_ptr(), fmt, W, H, t.stride(0) * t.element_size(), clear=CLEAR, wait_stream=stream, timings=True)
            kt = ctx.kernel_times()
            if i >= 5:
                per.append(sum(us for name, st, _s, us in kt if st == 4 and name.startswith("k_paint")))
        names = sorted({name for name, st, _s, _us in kt if st == 4})
        paint[fmt] = {"median_us": round(statistics.median(per), 2), "min_us": round(min(per), 2), "kernels": names}
    out["painter_us"] = paint
    for b in hosts:
        ctx.unregister_buffer(b)
    ctx.close()
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="paris-like-30k-4k,cubics-1080p")
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per workload child")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.frames, a.runs)
        return
    res = {"tool": "tools/device_target_bench.py", "results": []}
    for wl in a.workloads.split(","):
        p = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", wl,
                            "--frames", str(a.frames), "--runs", str(a.runs)], capture_output=True, text=True)
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode or not line:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            sys.exit(f"{wl}: child exited with {p.returncode}")   # (a fault or a time limit: nothing more runs on the GPU)
        res["results"].append(json.loads(line[0][7:]))
        print(json.dumps(res["results"][-1]))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
