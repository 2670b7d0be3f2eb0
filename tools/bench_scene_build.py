#!/usr/bin/env python3
"""Timing of ur_scene_build on one GPU (development aid; bench.py is the contract benchmark and never builds a scene).

    python tools/bench_scene_build.py [--draws 1000000] [--batches 9] [--iters 10] [--json out.jsonl]
    python tools/bench_scene_build.py --quick      # each shape a few times: for a rocprofv3 --kernel-trace --stats run

D draws over 4096 nodes and 64 meshes, 16 materials, the slots a permutation, stride 608. Over rotating output sets (cold: a set is
rewritten only after the others), in one process, alternating batch by batch:
  full build          bounds, centres, commands, one 608-byte record per draw and the summary: 720 bytes a draw
  transforms only     bounds, centres, World of each record and the summary: 112 bytes a draw
  fill 720 B / draw   a device fill of the full build's written bytes (torch's fill kernel on a buffer of that size): the store rate to hold it to
  fill 112 B / draw   the same for the update
  host build + upload ur_host_scene_build into host arrays, then the copies of bounds, commands, constants and centres to the device
Each device time is one event pair around a batch of back-to-back calls, divided by the calls (launch gaps included); the host time is
wall-clock around the call and the synchronised copies.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def tables_for(D, n_nodes=4096, n_meshes=64, n_materials=16, seed=1):
    from unclerenderer_amd import lib
    rng = np.random.default_rng(seed)
    f = np.float32
    nodes = np.zeros(n_nodes, np.dtype(lib.SceneNode))
    nodes["node_world"] = np.eye(4, dtype=f).reshape(-1)
    nodes["node_world"][:, 12:15] = rng.uniform(-100, 100, (n_nodes, 3))
    nodes["scale"] = rng.uniform(0.5, 2.0, (n_nodes, 3))
    nodes["max_scale"] = nodes["scale"].max(axis=1)
    angle = rng.uniform(0, 6.28, n_nodes).astype(f)
    nodes["rotation"] = np.stack([np.cos(angle), 0 * angle, -np.sin(angle), 0 * angle, 1 + 0 * angle, 0 * angle, np.sin(angle), 0 * angle, np.cos(angle)], axis=1)
    nodes["translate"] = rng.uniform(-10, 10, (n_nodes, 3))
    infos = np.zeros(n_meshes, np.dtype(lib.MeshInfo))
    infos["min"], infos["max"] = rng.uniform(-2, -1, (n_meshes, 3)), rng.uniform(1, 2, (n_meshes, 3))
    infos["center"] = f(0.5) * (infos["min"] + infos["max"])
    infos["radius"] = 2.0
    meshes = np.zeros(n_meshes, np.dtype(lib.SceneMesh))
    meshes["vertices"], meshes["indices"] = 0x7F0000000000 + np.arange(n_meshes) * 65536, 0x7E0000000000 + np.arange(n_meshes) * 65536
    meshes["vertex_bytes"], meshes["index_bytes"], meshes["stride"], meshes["index_format"] = 65536, 65536, 64, 42
    materials = np.zeros(n_materials, np.dtype(lib.SceneMaterialFactors))
    materials["BaseColor"] = rng.uniform(0, 1, (n_materials, 3))
    draws = np.zeros(D, np.dtype(lib.SceneDraw))
    draws["node"], draws["mesh"], draws["material"] = rng.integers(0, n_nodes, D), rng.integers(0, n_meshes, D), rng.integers(0, n_materials, D)
    draws["constants_slot"], draws["object_id"], draws["index_count"] = rng.permutation(D), np.arange(1, D + 1), 36
    return nodes, meshes, infos, materials, draws


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draws", type=int, default=1_000_000)
    ap.add_argument("--batches", type=int, default=9)
    ap.add_argument("--iters", type=int, default=10, help="calls per timed batch")
    ap.add_argument("--ring", type=int, default=4, help="output sets cycled through so that every call writes cold lines")
    ap.add_argument("--quick", action="store_true", help="each shape a few times (for the profiler run)")
    ap.add_argument("--json", default="", help="also append one JSON line per shape to this file")
    a = ap.parse_args()
    if a.quick:
        a.batches, a.iters, a.ring = 1, 3, 2
    import torch
    from unclerenderer_amd import hostmath, lib
    from unclerenderer_amd.hotpath import HotPath, SceneTables
    assert torch.cuda.is_available(), "bench_scene_build needs a GPU"
    hp = HotPath(0)
    D = a.draws
    host_tables = tables_for(D)
    dev = SceneTables(*host_tables, slot_count=D, constants_stride=608)
    frame = hostmath.build_frame_constants("sponza", 1920, 1080).scene
    sets = [hp.build_scene(dev, frame) for _ in range(a.ring)]
    fills = [(torch.empty(720 * D, dtype=torch.uint8, device="cuda"), torch.empty(112 * D, dtype=torch.uint8, device="cuda")) for _ in range(a.ring)]
    torch.cuda.synchronize()
    summary = sets[0].scene_summary()
    turn = [0]

    def pick(items):
        turn[0] += 1
        return items[turn[0] % a.ring]

    shapes = {"full build": lambda: hp.build_scene(dev, frame, out=pick(sets)),
              "transforms only": lambda: hp.build_scene(dev, frame, transforms_only=True, out=pick(sets)),
              "fill 720 B / draw": lambda: pick(fills)[0].fill_(7),
              "fill 112 B / draw": lambda: pick(fills)[1].fill_(7)}

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
    times = {k: [] for k in shapes}
    for _ in range(a.batches):
        for key, fn in shapes.items():
            times[key].append(time_batch(fn))

    # the host's way: the serial build into host arrays, then the uploads
    out = None
    host_times = []
    target = sets[0]
    for _ in range(1 if a.quick else 3):
        t0 = time.perf_counter()
        out = hostmath.scene_build(*host_tables, frame, D, 608, target.constants.data_ptr(), out=out)
        t1 = time.perf_counter()
        target.bounds.copy_(torch.from_numpy(out["bounds"]))
        target.commands.copy_(torch.from_numpy(out["commands"].view(np.int32)))
        target.constants.copy_(torch.from_numpy(out["constants"]))
        target.centers.copy_(torch.from_numpy(out["centers"]))
        torch.cuda.synchronize()
        host_times.append(((t1 - t0) * 1e6, (time.perf_counter() - t1) * 1e6))
    hp.close()

    rows = []
    for key, t in times.items():
        written = {"full build": 720, "transforms only": 112, "fill 720 B / draw": 720, "fill 112 B / draw": 112}[key] * D
        rows.append({"shape": f"{D} draws, {key}", "median_us": float(np.median(t)), "min_us": float(np.min(t)), "max_us": float(np.max(t)),
                     "written_GBps_at_median": written / float(np.median(t)) * 1e-3, "batches": len(t), "calls_per_batch": a.iters, "outputs": f"{a.ring} sets cycled (cold)"})
    totals = [b + u for b, u in host_times]
    rows.append({"shape": f"{D} draws, host build + upload", "median_us": float(np.median(totals)), "min_us": float(np.min(totals)), "max_us": float(np.max(totals)),
                 "build_us_median": float(np.median([b for b, _ in host_times])), "upload_us_median": float(np.median([u for _, u in host_times])), "batches": len(totals),
                 "calls_per_batch": 1, "outputs": "one set"})
    for r in rows:
        print(f"{r['shape']:48s} median {r['median_us']:12.2f} us  min {r['min_us']:12.2f} us")
    if a.json:
        with open(a.json, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    print(json.dumps({"tool": "bench_scene_build", "draws": D, "scene_radius": float(summary.scene_radius), "skipped": int(summary.skipped_draws), "quick": a.quick,
                      "results": rows}))


if __name__ == "__main__":
    main()
