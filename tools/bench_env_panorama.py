#!/usr/bin/env python3
"""Timing of ur_env_panorama on one GPU (development aid; bench.py is the contract benchmark and stages its cube once, before timing).

    python tools/bench_env_panorama.py [--batches 5] [--iters 4] [--json out.jsonl]
    python tools/bench_env_panorama.py --quick      # each shape once or twice, the host path on the small shape only

Two shapes at the recommended taps (ur_host_env_panorama_taps: 8 a side for both), seeded smooth panoramas, in one process, batch by batch:
  4096 x 2048 -> E = 512     33.5 MB of RGBE texels read, 12.6 MB of RGBA16F faces written, 1.6 M texels of 64 taps
  8192 x 4096 -> E = 1024    134 MB read, 50.3 MB written, 6.3 M texels of 64 taps
each beside
  device copy                a device-to-device copy of the bytes written: the store rate, to see how far from a copy the build is
  host path                  ur_hdr_unpack of a run-length coded file, ur_host_env_panorama (serial C++), then the upload of the faces, wall-clock
Each device time is one event pair around a batch of back-to-back calls, divided by the calls (launch gaps included). The device faces are
compared with the host's, byte for byte. No bound is asserted on the times: none has been promised.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

SHAPES = [(4096, 2048, 512), (8192, 4096, 1024)]


def smooth_panorama(w, h):
    """A sky gradient, a sun beyond fp16 and a ground, as RGBE texels [h, w, 4]."""
    az = ((np.arange(w) + 0.5) / w - 0.5) * 2 * np.pi
    el = (0.5 - (np.arange(h) + 0.5) / h) * np.pi
    up = np.sin(el)[:, None] * np.ones(w)[None, :]
    sun = np.cos(el)[:, None] * np.cos(az - 0.7)[None, :] * np.cos(0.6) + up * np.sin(0.6)
    rgb = np.stack([0.3 + 0.4 * np.maximum(up, 0) + 0.1 * np.cos(az)[None, :], 0.4 + 0.5 * np.maximum(up, 0), 0.5 + 0.9 * np.maximum(up, 0) - 0.3 * np.minimum(up, 0)], -1)
    rgb = rgb + (2.0e5 * np.maximum(sun, 0.0) ** 4096)[..., None]
    top = rgb.max(-1)
    _, ex = np.frexp(top)
    out = np.zeros((h, w, 4), np.uint8)
    out[..., :3] = np.minimum(np.rint(rgb * np.ldexp(1.0, 8 - ex)[..., None]), 255)
    out[..., 3] = ex + 128
    return out


def coded_file(rgbe):
    """The panorama as a .hdr file whose scanlines are run-length coded, all literal packets (what a noisy photograph gives)."""
    h, w = rgbe.shape[:2]
    packets = [(at, min(128, w - at)) for at in range(0, w, 128)]
    rows = []
    for y in range(h):
        row = [bytes((2, 2, w >> 8, w & 255))]
        for c in range(4):
            plane = rgbe[y, :, c].tobytes()
            row += [bytes((n,)) + plane[at:at + n] for at, n in packets]
        rows.append(b"".join(row))
    return b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y %d +X %d\n" % (h, w) + b"".join(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--iters", type=int, default=4, help="calls per timed batch")
    ap.add_argument("--quick", action="store_true", help="each shape once or twice; the host path on the small shape only")
    ap.add_argument("--json", default="", help="also append one JSON line per shape to this file")
    a = ap.parse_args()
    if a.quick:
        a.batches, a.iters = 1, 2
    import torch
    from unclerenderer_amd import assets, environment, hostmath
    from unclerenderer_amd.hotpath import HotPath, to_device
    assert torch.cuda.is_available(), "bench_env_panorama needs a GPU"
    hp = HotPath(0)

    def time_batch(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(a.iters):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) * 1e3 / a.iters

    rows, all_same = [], True
    for w, h, base in SHAPES:
        taps = hostmath.env_panorama_taps(w, h, base)
        name = f"{w} x {h} -> {base}, {taps} taps"
        pano = smooth_panorama(w, h)
        src = to_device(pano)
        dst = torch.empty((6, base, base, 4), dtype=torch.int16, device="cuda")
        other = torch.empty_like(dst)
        shapes = {f"device build {name}": lambda: environment.panorama_to_cube(hp, src, w, h, base, taps, out=dst),
                  f"device copy of {dst.numel() * 2} bytes": lambda: other.copy_(dst)}
        for fn in shapes.values():
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in shapes}
        for _ in range(a.batches):
            for key, fn in shapes.items():
                times[key].append(time_batch(fn))
        for key, t in times.items():
            rows.append({"shape": key, "median_us": float(np.median(t)), "min_us": float(np.min(t)), "max_us": float(np.max(t)),
                         "written_GBps_at_median": dst.numel() * 2 / float(np.median(t)) * 1e-3, "batches": len(t), "calls_per_batch": a.iters})
        if a.quick and base != SHAPES[0][2]:
            continue
        data = coded_file(pano)
        t0 = time.perf_counter()
        texels = assets.load_panorama_hdr(data)
        t1 = time.perf_counter()
        cube = hostmath.env_panorama(texels, w, h, base, taps)
        t2 = time.perf_counter()
        up = to_device(cube)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        same = bool(np.array_equal(texels, pano)) and bool(torch.equal(dst, up))
        all_same = all_same and same
        total = (t3 - t0) * 1e6
        rows.append({"shape": f"host path {name}: ur_hdr_unpack + ur_host_env_panorama + upload", "median_us": total, "min_us": total, "max_us": total,
                     "unpack_us": (t1 - t0) * 1e6, "build_us": (t2 - t1) * 1e6, "upload_us": (t3 - t2) * 1e6, "byte_equal_to_device": same, "batches": 1,
                     "calls_per_batch": 1})
    hp.close()
    for r in rows:
        print(f"{r['shape']:88s} median {r['median_us']:14.2f} us  min {r['min_us']:14.2f} us")
    if a.json:
        with open(a.json, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    print(json.dumps({"tool": "bench_env_panorama", "byte_equal_to_host": all_same, "quick": a.quick, "results": rows}))
    assert all_same, "the device faces' bytes are not ur_host_env_panorama's"


if __name__ == "__main__":
    main()
