#!/usr/bin/env python3
"""Timing of ur_env_prefilter on one GPU (development aid; bench.py is the contract benchmark and stages its cube once, before timing).

    python tools/bench_env_prefilter.py [--batches 5] [--iters 4] [--json out.jsonl]
    python tools/bench_env_prefilter.py --quick      # each shape once or twice: for a rocprofv3 --kernel-trace --stats run

On the top level of tests/golden/assets/output_pmrem.dds (256 x 256 faces, nine levels out), in one process, batch by batch:
  device prefilter S = 1024   ur_env_prefilter, the table already on the device: 3.1 MB read, the chain (4.2 MB) written
  device prefilter S = 256    the same with a quarter of the samples
  device copy                 a device-to-device copy of the chain's bytes: the store rate, to see how far from a copy the filter is
  host path S = 256           ur_host_env_prefilter (serial C++), then the upload of the chain, wall-clock; with --host-1024 also at
                              S = 1024 (four times as long)
Each device time is one event pair around a batch of back-to-back calls, divided by the calls (launch gaps included). The device chain is
compared with the host's at S = 256, byte for byte. No bound is asserted on the times: none has been promised.
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
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--iters", type=int, default=4, help="calls per timed batch")
    ap.add_argument("--quick", action="store_true", help="each shape once or twice (for the profiler run)")
    ap.add_argument("--host-1024", action="store_true", help="time the host path at S = 1024 too")
    ap.add_argument("--json", default="", help="also append one JSON line per shape to this file")
    a = ap.parse_args()
    if a.quick:
        a.batches, a.iters = 1, 2
    import torch
    from unclerenderer_amd import assets, hostmath, lib
    from unclerenderer_amd.hotpath import HotPath, to_device
    assert torch.cuda.is_available(), "bench_env_prefilter needs a GPU"
    hp = HotPath(0)
    top, base = assets.load_env_cube_top_level(CUBE)
    L = lib.load()
    chain_bytes = int(L.ur_env_cube_source_bytes(lib.UR_ENV_SOURCE_RGBA16F, base, base.bit_length()))
    src = to_device(top)
    tables = {s: to_device(hostmath.env_prefilter_table(base, s).copy()) for s in (1024, 256)}
    dst = torch.empty((chain_bytes // 8, 4), dtype=torch.int16, device="cuda")
    other = torch.empty_like(dst)
    scratch = torch.empty(int(L.ur_env_prefilter_scratch_bytes(base)), dtype=torch.uint8, device="cuda")

    shapes = {"device prefilter S = 1024": lambda: hp.prefilter_env_cube(src, base, 1024, table=tables[1024], out=dst, scratch=scratch),
              "device prefilter S = 256": lambda: hp.prefilter_env_cube(src, base, 256, table=tables[256], out=dst, scratch=scratch),
              "device copy": lambda: other.copy_(dst)}

    def time_batch(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(a.iters):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) * 1e3 / a.iters

    for fn in shapes.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in shapes}
    for _ in range(a.batches):
        for key, fn in shapes.items():
            times[key].append(time_batch(fn))

    host_times, same = {}, None
    for samples in (256, 1024) if a.host_1024 else (256,):
        table = hostmath.env_prefilter_table(base, samples)
        t0 = time.perf_counter()
        chain = hostmath.env_prefilter(top, base, samples, table=table)
        t1 = time.perf_counter()
        up = to_device(chain)
        torch.cuda.synchronize()
        host_times[samples] = ((t1 - t0) * 1e6, (time.perf_counter() - t1) * 1e6)
        if samples == 256:
            shapes["device prefilter S = 256"]()
            torch.cuda.synchronize()
            same = bool(torch.equal(dst, up))
    hp.close()

    rows = []
    for key, t in times.items():
        rows.append({"shape": key, "median_us": float(np.median(t)), "min_us": float(np.min(t)), "max_us": float(np.max(t)),
                     "written_GBps_at_median": chain_bytes / float(np.median(t)) * 1e-3, "batches": len(t), "calls_per_batch": a.iters})
    for samples, (filt, up) in host_times.items():
        rows.append({"shape": f"host path S = {samples}: ur_host_env_prefilter + upload", "median_us": filt + up, "min_us": filt + up, "max_us": filt + up,
                     "filter_us": filt, "upload_us": up, "batches": 1, "calls_per_batch": 1})
    for r in rows:
        print(f"{r['shape']:56s} median {r['median_us']:14.2f} us  min {r['min_us']:14.2f} us")
    if a.json:
        with open(a.json, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    print(json.dumps({"tool": "bench_env_prefilter", "cube": f"{base}, {base.bit_length()} levels", "chain_bytes": chain_bytes, "byte_equal_to_host_at_256": same,
                      "quick": a.quick, "results": rows}))
    assert same, "the device chain's bytes are not ur_host_env_prefilter's"


if __name__ == "__main__":
    main()
