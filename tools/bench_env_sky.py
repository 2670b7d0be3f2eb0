#!/usr/bin/env python3
"""Timing of ur_env_sky, ur_brdf_lut and environment.bake_sky on one GPU (development aid; bench.py is the contract benchmark and makes
its tables once, before timing).

    python tools/bench_env_sky.py [--batches 5] [--iters 8] [--json out.jsonl]
    python tools/bench_env_sky.py --step sky-256-1          # one step alone, in this process

Without --step every step runs one after the other, each in a child process of its own under its own time limit; the first one that
fails or runs out of time ends the run. The steps:
  sky-E-K       ur_env_sky at edge E (256, 512) with K taps a side (1, 4): 48 E^2 bytes of RGBA16F faces written, nothing read
  lut           ur_brdf_lut at 128 x 32 with 1024 samples: 512 KB of table read, 16 KB written
  bake-256      environment.bake_sky at edge 256, 1024 samples: the capture, the prefilter and the cube build
each beside
  device copy   a device-to-device copy of the bytes written: the store rate, to see how far from a copy the call is
  host route    the serial C++ twin (ur_host_env_sky; ur_host_brdf_lut_table + ur_host_brdf_lut; + ur_host_env_prefilter and
                ur_stage_env_cube for the bake), then the upload, wall-clock
Each device time is one event pair around a batch of back-to-back calls, divided by the calls (launch gaps included). The device bytes
are compared with the host's. No bound is asserted on the times: none has been promised, these are load-time calls.
"""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

# step -> its time limit in seconds (the bake's host route is about 6 s of serial prefilter)
STEPS = {"sky-256-1": 120, "sky-256-4": 120, "sky-512-1": 120, "sky-512-4": 120, "lut": 120, "bake-256": 240}
SUN, COLOR, CAMERA_Y = (0.3, 0.8, -0.5), (1.0, 0.95, 0.9), 1.5


def sky_constants():
    from unclerenderer_amd import lib
    sky = lib.SkyConstants()
    sky.CameraPosition[1] = CAMERA_Y
    sky.LightDirection[:], sky.LightColor[:] = list(SUN), list(COLOR)
    return sky


def run_step(step, a):
    import torch
    from unclerenderer_amd import environment, hostmath
    from unclerenderer_amd.hotpath import HotPath, to_device
    assert torch.cuda.is_available(), "bench_env_sky needs a GPU"
    hp = HotPath(0)
    sky = sky_constants()

    def time_batch(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(a.iters):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) * 1e3 / a.iters

    t0 = time.perf_counter()
    if step.startswith("sky-"):
        base, taps = (int(v) for v in step.split("-")[1:])
        name = f"ur_env_sky, edge {base}, {taps} taps a side"
        dst = torch.empty((6, base, base, 4), dtype=torch.int16, device="cuda")
        call = lambda: environment.sky_to_cube(hp, sky, base, taps, out=dst)  # noqa: E731
        host = hostmath.env_sky(sky, base, taps)
        t1 = time.perf_counter()
        up = to_device(host)
    elif step == "lut":
        name = "ur_brdf_lut, 128 x 32, 1024 samples"
        table = to_device(hostmath.brdf_lut_table(32, 1024).copy())
        dst = torch.empty((32, 128, 2), dtype=torch.int16, device="cuda")
        from unclerenderer_amd import lib
        from unclerenderer_amd.hotpath.tensors import _ptr, nbytes
        call = lambda: lib.check(hp._L.ur_brdf_lut(hp._ctx, 128, 32, 1024, _ptr(table), nbytes(table), _ptr(dst), nbytes(dst)), "ur_brdf_lut")  # noqa: E731
        t0 = time.perf_counter()
        host = hostmath.brdf_lut(128, 32, 1024)
        t1 = time.perf_counter()
        up = to_device(host)
    else:
        base = int(step.split("-")[1])
        name = f"environment.bake_sky, edge {base}, 1024 samples"
        dst = environment.bake_sky(hp, sky, base, 1024)
        call = lambda: environment.bake_sky(hp, sky, base, 1024, out=dst)  # noqa: E731
        t0 = time.perf_counter()
        payload = hostmath.env_prefilter(hostmath.env_sky(sky, base, 1), base, 1024)
        t1 = time.perf_counter()
        up = hp.stage_env_cube(payload, base, base.bit_length())
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    other = torch.empty_like(dst)
    shapes = {name: call, f"device copy of {dst.numel() * dst.element_size()} bytes": lambda: other.copy_(dst)}
    for fn in shapes.values():
        fn()
    torch.cuda.synchronize()
    same = bool(torch.equal(dst.view(torch.uint8).reshape(-1), up.view(torch.uint8).reshape(-1)))
    times = {k: [] for k in shapes}
    for _ in range(a.batches):
        for key, fn in shapes.items():
            times[key].append(time_batch(fn))
    rows = [{"step": step, "shape": key, "median_us": float(np.median(t)), "min_us": float(np.min(t)), "max_us": float(np.max(t)), "batches": len(t),
             "calls_per_batch": a.iters} for key, t in times.items()]
    rows.append({"step": step, "shape": f"host route of {name} + upload", "median_us": (t2 - t0) * 1e6, "min_us": (t2 - t0) * 1e6, "max_us": (t2 - t0) * 1e6,
                 "build_us": (t1 - t0) * 1e6, "upload_us": (t2 - t1) * 1e6, "byte_equal_to_device": same, "batches": 1, "calls_per_batch": 1})
    hp.close()
    for r in rows:
        print(f"{r['shape']:72s} median {r['median_us']:14.2f} us  min {r['min_us']:14.2f} us")
    if a.json:
        with open(a.json, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    print(json.dumps({"tool": "bench_env_sky", "step": step, "byte_equal_to_host": same, "results": rows}))
    assert same, "the device bytes are not the host route's"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--iters", type=int, default=8, help="calls per timed batch")
    ap.add_argument("--step", default="", choices=[""] + list(STEPS), help="run this step alone, in this process")
    ap.add_argument("--json", default="", help="also append one JSON line per row to this file")
    a = ap.parse_args()
    if a.step:
        return run_step(a.step, a)
    for step, limit in STEPS.items():  # a child each, under its own limit; nothing more is started after a failure
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, str(Path(__file__).resolve()), "--step", step, "--batches", str(a.batches), "--iters", str(a.iters)]
        r = subprocess.run(cmd + (["--json", a.json] if a.json else []))
        if r.returncode != 0:
            sys.exit(f"bench_env_sky: step {step} ended with {r.returncode}; nothing more is run")


if __name__ == "__main__":
    main()
