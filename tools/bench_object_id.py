#!/usr/bin/env python3
"""Timing of the ObjectId pass (ur_object_id_pass) and the pick (ur_object_id_pick) on one GPU (development aid; bench.py is the contract
benchmark and never draws).

    python tools/bench_object_id.py [--batches 7] [--iters 10] [--json out.jsonl]
    python tools/bench_object_id.py --raster-part-only --json parent.jsonl   # with UR_HOTPATH_LIB=<a build without the ObjectId calls>
    python tools/bench_object_id.py --json out.jsonl --check-against parent.jsonl

At 3840 x 2160, tools/bench_shadow.py's small workload - 1 M triangles of 1/8 px to 8 px - cut into 8 commands, over cold target sets (a
ring of depth images, each ur_depth_prepass' of these draws, with their own keys, ObjectId images and pick records). Each time is one
device-event pair around a batch of back-to-back calls, divided by the calls (launch gaps included); batch by batch in the same process:
  the image pass           ur_object_id_pass: clear of the keys, raster, queue, ObjectId resolve;
  the pick, 1 point        ur_object_id_pick: clear of the records, pick kernel, finish;
  the pick, 64 points
  the raster part          ur_gbuffer_pass_parts(UR_GBUFFER_PART_RASTER): the clear, the raster and the queue - the yardstick, which an
                           earlier build of the library has too.
--raster-part-only times the yardstick alone and binds nothing else, so that it runs on a library built from the parent commit
(UR_HOTPATH_LIB): alternate the two in one visit and append both to their files.

--check-against FILE asserts the one bound the pick is held to: the median of the 1-point pick's batches (every row of --json's file) is at
most the median of FILE's raster-part batches plus their spread, the largest minus the smallest batch. Per triangle the pick does the
raster's front half and one box test, serves no fragment and clears nothing: more time than the raster part means a mistake in the kernel.
No other ratio is promised; the other rows are written down as measured."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
W, H = 3840, 2160
NEW = ("ur_object_id_pass", "ur_object_id_pick")
PICK_1, RASTER_PART = "the pick, 1 point", "the raster part (ur_gbuffer_pass_parts)"


def batches_of(path, shape):
    out = []
    for line in Path(path).read_text().splitlines():
        r = json.loads(line)
        if r.get("tool") == "bench_object_id" and r["shape"].endswith(shape):
            out += r["batch_us"]
    return out


def check(own, parent):
    pick, raster = batches_of(own, PICK_1), batches_of(parent, RASTER_PART)
    assert pick and raster, "no 1-point pick rows, or no raster-part rows of the parent build"
    spread = max(raster) - min(raster)
    bound = float(np.median(raster)) + spread
    print(f"1-point pick: median {np.median(pick):.2f} us over {len(pick)} batches; the parent's raster part: median {np.median(raster):.2f} us over {len(raster)} batches, "
          f"spread {spread:.2f} us: bound {bound:.2f} us")
    assert float(np.median(pick)) <= bound, "the 1-point pick is slower than the parent's raster part"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10, help="calls per timed batch")
    ap.add_argument("--ring", type=int, default=4, help="target sets cycled through so that every call meets cold targets")
    ap.add_argument("--small", type=int, default=1_000_000)
    ap.add_argument("--reserve", type=int, default=1 << 19)
    ap.add_argument("--raster-part-only", action="store_true", help="the yardstick alone: runs on a library without the ObjectId entry points")
    ap.add_argument("--json", default="")
    ap.add_argument("--check-against", default="", help="a --raster-part-only file of the parent build: assert the 1-point pick's bound")
    a = ap.parse_args()
    import torch
    from bench_shadow import PROJ, VIEW, camera_space, time_batch, triangles
    from unclerenderer_amd import lib
    if a.raster_part_only:
        for name in NEW:
            lib.SIGNATURES.pop(name, None)
    from unclerenderer_amd.hotpath import HotPath, gbuffer_targets, pack_draw_commands, raster_draws, to_device
    assert torch.cuda.is_available(), "bench_object_id needs a GPU"
    hp = HotPath(0)
    rng = np.random.default_rng(2163)
    cb = np.zeros(152, np.float32)
    cb[:16] = np.eye(4, dtype=np.float32).reshape(-1)
    cb[64:68], cb[80:83], cb[104], cb[105] = (0.8, 0.7, 0.6, 1.0), (0.1, 0.2, 0.3), 0.25, 0.5
    pos = camera_space(triangles(rng, a.small, 0.125, 8.0, W, H))
    v = np.zeros((pos.shape[0], 16), np.float32)
    v[:, :3], v[:, 5], v[:, 12:16] = pos, -1.0, 1.0
    vb, ib = to_device(v.reshape(-1)), to_device(np.arange(pos.shape[0], dtype=np.uint32))
    n = 8
    cuts = (np.linspace(0, pos.shape[0] // 3, n + 1).astype(int) * 3).tolist()
    blocks = []
    for k in range(n):
        c = cb.copy()
        c.view(np.uint32)[148] = 100 + k
        blocks.append(to_device(c))
    cmds = to_device(pack_draw_commands([dict(vertices=vb, indices=ib, constants=blocks[k], stride=64, start_index=cuts[k], index_count=cuts[k + 1] - cuts[k]) for k in range(n)]))
    draws = raster_draws(cmds)
    half = [torch.empty((H, W, 4), dtype=torch.float16, device="cuda") for _ in range(3)]  # (the raster part leaves them alone: one set serves the ring)
    gc = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    sets = []
    for _ in range(a.ring):
        depth = torch.zeros((H, W), dtype=torch.float32, device="cuda")
        keys, oid = (torch.zeros((H, W), dtype=torch.int32, device="cuda") for _ in range(2))
        sets.append(dict(depth=depth, keys=keys, oid=oid, targets=gbuffer_targets(half[0], half[1], gc, half[2], keys), records=torch.zeros((64, 4), dtype=torch.int32, device="cuda")))
    hp.raster_reserve(a.reserve)
    for s in sets:
        hp.depth_prepass(VIEW, PROJ, cmds, s["depth"])
    points = np.stack([rng.integers(0, W, 64), rng.integers(0, H, 64)], axis=1)
    stats = torch.zeros(6, dtype=torch.int32, device="cuda")

    def raster_part(i, st=None):
        s = sets[i % a.ring]
        hp.gbuffer_pass(VIEW, PROJ, cmds, s["depth"], s["targets"], W, H, parts=lib.UR_GBUFFER_PART_RASTER, stats=st)

    fns = {RASTER_PART: raster_part}
    if not a.raster_part_only:
        fns = {"the image pass (ur_object_id_pass)": lambda i, st=None: hp.object_id_pass(draws, VIEW, PROJ, sets[i % a.ring]["depth"], W, H, object_id=sets[i % a.ring]["oid"],
                                                                                         keys=sets[i % a.ring]["keys"], stats=st),
               PICK_1: lambda i, st=None: hp.object_id_pick(draws, VIEW, PROJ, sets[i % a.ring]["depth"], W, H, points[:1], results=sets[i % a.ring]["records"][:1], stats=st),
               "the pick, 64 points": lambda i, st=None: hp.object_id_pick(draws, VIEW, PROJ, sets[i % a.ring]["depth"], W, H, points, results=sets[i % a.ring]["records"], stats=st),
               **fns}
    seen = {}
    for k, f in fns.items():
        stats.zero_()
        f(0, stats)
        torch.cuda.synchronize()
        seen[k] = stats.cpu().numpy().view(np.uint32).tolist()
    times = {k: [] for k in fns}
    for _ in range(a.batches):
        for k, f in fns.items():
            times[k].append(time_batch(torch, f, a.iters))
    picked = int((sets[0]["records"][:, 1] != 0).sum()) if not a.raster_part_only else 0
    hp.raster_reserve(0)
    hp.close()
    rows = [{"tool": "bench_object_id", "library": str(lib.library_path()), "shape": f"{W}x{H}, small in {n} commands, {k}", "median_us": float(np.median(t)), "min_us": float(np.min(t)),
             "max_us": float(np.max(t)), "batch_us": [float(x) for x in t], "stats_one_call": seen[k], "batches": len(t), "calls_per_batch": a.iters, "sets": a.ring,
             "points_that_hit": picked} for k, t in times.items()]
    for r in rows:
        print(f"{r['shape']:80s} median {r['median_us']:10.2f} us  min {r['min_us']:10.2f} us  max {r['max_us']:10.2f} us  stats {r['stats_one_call']}")
    if a.json:
        with open(a.json, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    print(json.dumps({"tool": "bench_object_id", "results": rows}))
    if a.check_against:
        assert a.json, "--check-against reads this run's rows from --json's file"
        check(a.json, a.check_against)


if __name__ == "__main__":
    main()
