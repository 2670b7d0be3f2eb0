#!/usr/bin/env python3
"""Timing of ur_env_cube_build on one GPU (development aid; bench.py is the contract benchmark and stages its cube once, before timing).

    python tools/bench_env_cube.py [--batches 7] [--iters 10] [--json out.jsonl]
    python tools/bench_env_cube.py --quick      # each shape a few times: for a rocprofv3 --kernel-trace --stats run

On tests/golden/assets/output_pmrem.dds (256, 9 levels, BC6H_SF16) and on its RGBA16F twin (the same cube decoded), in one process,
alternating batch by batch over rotating destinations (cold: a destination is rewritten only after the others):
  device build BC6H_SF16   ur_env_cube_build of the file's payload: 0.5 MB read, the staged cube (about 10.7 MB) written
  device build RGBA16F     the same over decoded texels: 4.2 MB read
  device copy              a device-to-device copy of the staged cube's bytes: the store rate to hold the build to
  host path                the way it went before: ur_dds_decode_rgba16f of the file, then ur_stage_env_cube (border fold and row pairs
                           on the host, one synchronous copy), wall-clock
Each device time is one event pair around a batch of back-to-back calls, divided by the calls (launch gaps included). One bound is
asserted: the device build's median (BC6H_SF16, the shipped form) is at most the host path's median of the same run.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
CUBE = ROOT / "tests" / "golden" / "assets" / "output_pmrem.dds"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10, help="calls per timed batch")
    ap.add_argument("--ring", type=int, default=4, help="destinations cycled through so that every call writes cold lines")
    ap.add_argument("--quick", action="store_true", help="each shape a few times (for the profiler run)")
    ap.add_argument("--json", default="", help="also append one JSON line per shape to this file")
    a = ap.parse_args()
    if a.quick:
        a.batches, a.iters, a.ring = 1, 3, 2
    import torch
    from unclerenderer_amd import assets, lib
    from unclerenderer_amd.hotpath import HotPath, to_device
    assert torch.cuda.is_available(), "bench_env_cube needs a GPU"
    hp = HotPath(0)
    payload, fmt, base, mips = assets.load_env_cube_dds_source(CUBE)
    texels, _, _, _ = assets.load_env_cube_dds(CUBE)
    blocks, halves = to_device(payload), to_device(texels.view(np.uint8).reshape(-1))
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    n = int(lib.load().ur_env_cube_texels(base, mips))
    ring = [torch.empty((n, 4), dtype=torch.int16, device="cuda") for _ in range(a.ring)]
    source = hp.stage_env_cube(texels, base, mips)
    torch.cuda.synchronize()
    turn = [0]

    def pick():
        turn[0] += 1
        return ring[turn[0] % a.ring]

    shapes = {"device build BC6H_SF16": lambda: hp.build_env_cube(blocks, fmt, base, mips, info, out=pick()),
              "device build RGBA16F": lambda: hp.build_env_cube(halves, lib.UR_ENV_SOURCE_RGBA16F, base, mips, info, out=pick()),
              "device copy": lambda: pick().copy_(source)}

    def time_batch(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(a.iters):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) * 1e3 / a.iters

    for fn in shapes.values():
        for _ in range(a.ring):
            fn()
    torch.cuda.synchronize()
    same = all(torch.equal(t, source) for t in ring)  # what was timed is the staged cube
    times = {k: [] for k in shapes}
    for _ in range(a.batches):
        for key, fn in shapes.items():
            times[key].append(time_batch(fn))

    # the way it went before: decode on the host, stage on the host, one blocking copy
    host_times = []
    for _ in range(1 if a.quick else 5):
        t0 = time.perf_counter()
        decoded, b, m, _ = assets.load_env_cube_dds(CUBE)
        t1 = time.perf_counter()
        hp.stage_env_cube(decoded, b, m)
        torch.cuda.synchronize()
        host_times.append(((t1 - t0) * 1e6, (time.perf_counter() - t1) * 1e6))
    hp.close()

    rows = []
    for key, t in times.items():
        rows.append({"shape": key, "median_us": float(np.median(t)), "min_us": float(np.min(t)), "max_us": float(np.max(t)),
                     "written_GBps_at_median": 8 * n / float(np.median(t)) * 1e-3, "batches": len(t), "calls_per_batch": a.iters, "outputs": f"{a.ring} destinations cycled (cold)"})
    totals = [d + s for d, s in host_times]
    rows.append({"shape": "host path: decode + ur_stage_env_cube", "median_us": float(np.median(totals)), "min_us": float(np.min(totals)), "max_us": float(np.max(totals)),
                 "decode_us_median": float(np.median([d for d, _ in host_times])), "stage_us_median": float(np.median([s for _, s in host_times])), "batches": len(totals),
                 "calls_per_batch": 1, "outputs": "a fresh destination each"})
    for r in rows:
        print(f"{r['shape']:44s} median {r['median_us']:12.2f} us  min {r['min_us']:12.2f} us")
    if a.json:
        with open(a.json, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    device, host = rows[0]["median_us"], rows[-1]["median_us"]
    print(json.dumps({"tool": "bench_env_cube", "cube": f"{base}, {mips} levels, format {fmt}", "staged_bytes": 8 * n, "byte_equal_to_stage_env_cube": same,
                      "host_over_device": host / device, "quick": a.quick, "results": rows}))
    assert same, "the device build's bytes are not ur_stage_env_cube's"
    assert device <= host, f"the device build's median ({device:.1f} us) is above the host path's ({host:.1f} us)"


if __name__ == "__main__":
    main()
