#!/usr/bin/env python3
"""Time ur_texture_transcode against its two yardsticks, in one process.

    python tools/bench_texture_transcode.py [--sizes 1024,4096] [--batches 7] [--iters 10] [--ring 4] [--host-calls 2] [--json out.jsonl]

Per size (a square texture with its full mip chain) and per source format (BC1, BC3, BC7; random blocks, BC7 cycling through its eight
modes), three legs:

  transcode  one ur_texture_transcode call: the source chain's bytes read, the RGBA8 chain's bytes written.
  copy       a device-to-device copy of the destination's byte count: the floor for writing 4 bytes a texel (it reads as many bytes
             as it writes, so it moves more than the transcode does).
  host       the host route for the same chain: ur_host_texture_decode_level per level, then the upload of the RGBA8 chain; wall
             clock around --host-calls calls that end in a device synchronise (one CPU thread; it is a load-time cost, not a kernel).

transcode and copy: each time is one device-event pair around a batch of --iters back-to-back calls over --ring rotating buffer sets
(every call meets buffers that the calls before it pushed out of the caches), divided by the calls; --batches batches, taken leg by leg
in turn; median and minimum. Before timing, the transcode's output is compared byte for byte with the host route's chain.
Needs a GPU: there is no fallback."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
FORMATS = (("BC1", 71), ("BC3", 77), ("BC7", 98))


def time_batch(torch, fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for k in range(iters):
        fn(k)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def random_chain(rng, fmt: int, nbytes: int) -> np.ndarray:
    data = rng.integers(0, 256, nbytes, dtype=np.uint8)
    if fmt == 98:  # plain random bytes are mode 0 half the time: block i gets the mode bits of mode i % 8
        b = data.reshape(-1, 16)
        m = np.arange(b.shape[0]) % 8
        b[:, 0] = (b[:, 0] & ~((2 << m) - 1) & 255) | (1 << m)
    return data


def host_route(hostmath, torch, fmt, data, size, mips, per):
    """The chain decoded level by level on the host and uploaded: (device tensor, seconds)."""
    t0 = time.perf_counter()
    levels, at = [], 0
    for k in range(mips):
        s = max(1, size >> k)
        levels.append(hostmath.texture_decode_level(fmt, data[at:], s, s).reshape(-1))
        at += ((s + 3) >> 2) ** 2 * per
    dev = torch.from_numpy(np.concatenate(levels)).to("cuda")
    torch.cuda.synchronize()
    return dev, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="1024,4096")
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10, help="calls per timed batch")
    ap.add_argument("--ring", type=int, default=4, help="buffer sets cycled through so that every call meets cold buffers")
    ap.add_argument("--host-calls", type=int, default=2)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    from unclerenderer_amd import hostmath, lib
    from unclerenderer_amd.hotpath import HotPath
    hp = HotPath(0)
    L = lib.load()
    rng = np.random.default_rng(315)
    rows = []
    for size in [int(s) for s in a.sizes.split(",")]:
        mips = size.bit_length()
        dst_bytes = int(L.ur_texture_transcode_bytes(size, size, mips))
        for name, fmt in FORMATS:
            per = 8 if fmt == 71 else 16
            src_bytes = hostmath.texture_chain_bytes(fmt, size, size, mips)
            chains = [random_chain(rng, fmt, src_bytes) for _ in range(a.ring)]
            src = [torch.from_numpy(c).to("cuda") for c in chains]
            dst = [torch.empty(dst_bytes // 4, dtype=torch.int32, device="cuda") for _ in range(a.ring)]
            other = [torch.empty(dst_bytes // 4, dtype=torch.int32, device="cuda") for _ in range(a.ring)]

            def transcode(k):
                i = k % a.ring
                lib.check(L.ur_texture_transcode(hp.ctx, fmt, src[i].data_ptr(), size, size, mips, dst[i].data_ptr(), None), "ur_texture_transcode")

            def copy(k):
                i = k % a.ring
                other[i].copy_(dst[(i + 1) % a.ring])

            # the results first: the device's chain against the host route's, byte for byte (this also warms every set up)
            host_s = []
            for n in range(max(1, a.host_calls)):
                want, seconds = host_route(hostmath, torch, fmt, chains[n % a.ring], size, mips, per)
                host_s.append(seconds)
                transcode(n % a.ring)
                torch.cuda.synchronize()
                if not torch.equal(dst[n % a.ring].view(torch.uint8), want):
                    raise SystemExit(f"{name} {size}: the transcoded chain differs from the host route's")
                del want
            for k in range(a.ring):
                transcode(k), copy(k)
            torch.cuda.synchronize()
            times = {"transcode": [], "copy": []}
            for _ in range(a.batches):
                for leg, fn in (("transcode", transcode), ("copy", copy)):
                    times[leg].append(time_batch(torch, fn, a.iters))
            t, c = times["transcode"], times["copy"]
            row = {"shape": f"{size}x{size}, {mips} mips, {name}", "source_bytes": src_bytes, "rgba8_bytes": dst_bytes,
                   "transcode_median_us": float(np.median(t)), "transcode_min_us": float(np.min(t)), "transcode_max_us": float(np.max(t)),
                   "copy_median_us": float(np.median(c)), "copy_min_us": float(np.min(c)), "copy_max_us": float(np.max(c)),
                   "transcode_over_copy": float(np.median(t) / np.median(c)),
                   "transcode_gb_per_s": (src_bytes + dst_bytes) / np.median(t) * 1e-3, "copy_gb_per_s": 2 * dst_bytes / np.median(c) * 1e-3,
                   "host_route_median_ms": float(np.median(host_s)) * 1e3, "host_route_min_ms": float(np.min(host_s)) * 1e3, "host_calls": len(host_s),
                   "batches": a.batches, "calls_per_batch": a.iters, "ring": a.ring}
            rows.append(row)
            print(f"{row['shape']:28s} transcode median {row['transcode_median_us']:9.2f} us min {row['transcode_min_us']:9.2f} us ({row['transcode_gb_per_s']:7.1f} GB/s)   "
                  f"copy median {row['copy_median_us']:9.2f} us min {row['copy_min_us']:9.2f} us ({row['copy_gb_per_s']:7.1f} GB/s)   x{row['transcode_over_copy']:.2f}   "
                  f"host route median {row['host_route_median_ms']:9.1f} ms of {len(host_s)}", flush=True)
            del src, dst, other
            torch.cuda.empty_cache()
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        with open(a.json, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    hp.close()


if __name__ == "__main__":
    main()
