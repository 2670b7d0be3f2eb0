"""Times ur_mesh_build in one process over a generated grid mesh of about 1 M triangles, three configurations:
tangents absent (the tangent pass runs), tangents present (assembly and expansion alone), and the first with a fan of 100 000 triangles
around one vertex appended (the long-segment queue). Per configuration: the device build (median and minimum of batches, events on the
stream), beside it a device copy of the bytes the build writes, and ur_host_mesh_build plus the upload of its result.

    python tools/bench_mesh_build.py [--side 708] [--batches 7] [--per-batch 3]

Prints one JSON line per configuration. No ratio is asserted."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def grid_mesh(side, tangents, fan):
    from unclerenderer_amd import hostmath
    rng = np.random.default_rng(1)
    ys, xs = np.mgrid[0:side, 0:side]
    p = np.stack([xs, ys, np.zeros_like(xs)], -1).reshape(-1, 3).astype(np.float32)
    p += rng.uniform(-0.3, 0.3, p.shape).astype(np.float32)
    a = (ys[:-1, :-1] * side + xs[:-1, :-1]).reshape(-1)
    idx = np.stack([a, a + 1, a + side + 1, a, a + side + 1, a + side], 1).reshape(-1)
    if fan:
        ring = 1 + np.arange(fan + 1) % (side * side - 1)
        idx = np.concatenate([idx, np.stack([np.zeros(fan, np.int64), ring[:-1], ring[1:]], 1).reshape(-1)])
    n = np.tile(np.float32([0, 0, 1]), (len(p), 1))
    uv = (p[:, :2] / np.float32(side)).astype(np.float32)
    parts = [p, n, uv] + ([np.tile(np.float32([1, 0, 0, 1]), (len(p), 1))] if tangents else [])
    blob, offsets = b"", []
    for part in parts:
        offsets.append(len(blob))
        blob += part.astype("<f4").tobytes()
    index_offset = len(blob)
    blob += idx.astype("<u4").tobytes()
    prim = hostmath.mesh_primitive(len(p), (offsets[0], 12), (index_offset, idx.size, 5125), normal=(offsets[1], 12), texcoord=(offsets[2], 8),
                                   tangent=(offsets[3], 16) if tangents else None)
    return np.frombuffer(blob, np.uint8), [prim]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=708)  # 707^2 * 2 = 999 698 triangles
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--per-batch", type=int, default=3)
    args = ap.parse_args()
    import torch
    from unclerenderer_amd import hostmath
    from unclerenderer_amd.hotpath import HotPath, to_device
    hp = HotPath(0)
    for name, tangents, fan in (("tangents absent", False, 0), ("tangents present", True, 0), ("tangents absent, fan of 100000", False, 100000)):
        data, prims = grid_mesh(args.side, tangents, fan)
        layout, _ = hostmath.mesh_layout(prims, data.size)
        buffer = to_device(data.copy())
        scratch = torch.empty(int(layout.scratch_bytes), dtype=torch.uint8, device="cuda")
        written = 64 * layout.vertex_count + 4 * layout.index_count
        src, dst = torch.empty(written, dtype=torch.uint8, device="cuda"), torch.empty(written, dtype=torch.uint8, device="cuda")

        def timed(fn):
            fn()
            torch.cuda.synchronize()
            times = []
            for _ in range(args.batches):
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record(torch.cuda.current_stream())
                for _ in range(args.per_batch):
                    fn()
                stop.record(torch.cuda.current_stream())
                stop.synchronize()
                times.append(start.elapsed_time(stop) / args.per_batch)
            return float(np.median(times)), float(np.min(times))

        build_ms = timed(lambda: hp.build_mesh(buffer, prims, scratch=scratch))
        copy_ms = timed(lambda: dst.copy_(src))
        t0 = time.perf_counter()
        vertices, indices, _, info = hostmath.mesh_build(data, prims)
        t1 = time.perf_counter()
        to_device(vertices), to_device(indices)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        print(json.dumps({"configuration": name, "vertices": layout.vertex_count, "triangles": layout.index_count // 3, "bytes_written": written,
                          "device_build_ms_median": build_ms[0], "device_build_ms_min": build_ms[1], "device_copy_ms_median": copy_ms[0], "device_copy_ms_min": copy_ms[1],
                          "host_build_ms": 1e3 * (t1 - t0), "host_upload_ms": 1e3 * (t2 - t1), "tangents_regenerated": int(info.tangents_regenerated),
                          "batches": args.batches, "per_batch": args.per_batch}), flush=True)
    hp.close()


if __name__ == "__main__":
    main()
