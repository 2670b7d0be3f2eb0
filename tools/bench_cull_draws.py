#!/usr/bin/env python3
"""Timing of the cull with and without draw ranges (ur_cull_indirect_args_draws) on one GPU (development aid; bench.py is the
contract benchmark and never sets ranges).

    python tools/bench_cull_draws.py [--batches 9] [--iters 30] [--json out.jsonl]
    python tools/bench_cull_draws.py --quick      # each shape a few times: for a rocprofv3 --kernel-trace --stats run

C5 (BASELINE config 5): 1 M instance AABBs against the 12-mip HZB of a 7680x4320 depth, with the visible list, over six rotating
buffer sets (bounds, commands, list and compacted commands: cold, as bench.py's extras) - without ranges, then with R = 1, 64,
4096 (a random partition) and one range per command, the shapes alternating batch by batch in one process. Then the single-block
calls of Sponza's 25 and pica_pica's 170 commands, without ranges and with one range per command. Each time is one device-event
pair around a batch of back-to-back calls, divided by the calls (launch gaps included). Kernel times and launch counts come from a
separate rocprofv3 --kernel-trace --stats run of --quick.
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def time_batch(torch, fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for k in range(iters):
        fn(k)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=1_000_000)
    ap.add_argument("--batches", type=int, default=9)
    ap.add_argument("--iters", type=int, default=30, help="calls per timed batch")
    ap.add_argument("--ring", type=int, default=6, help="buffer sets cycled through so that every call meets cold inputs")
    ap.add_argument("--quick", action="store_true", help="each shape a few times (for the profiler run)")
    ap.add_argument("--json", default="", help="also append one JSON line per shape to this file")
    a = ap.parse_args()
    if a.quick:
        a.batches, a.iters, a.ring = 1, 3, 2
    import torch
    from unclerenderer_amd import hostmath, scene, synth
    from unclerenderer_amd.hotpath import HotPath, HzbLayout, to_device
    assert torch.cuda.is_available(), "bench_cull_draws needs a GPU"
    hp = HotPath(0)
    n = a.instances
    W8, H8 = 7680, 4320
    fc8 = hostmath.build_frame_constants("sponza", W8, H8)
    lay8 = HzbLayout(W8, H8)
    g8 = synth.gbuffer_scene(fc8.view, fc8.proj, fc8.camera_position, W8, H8, synth.SEED_BASE + 5)
    hzb8 = torch.zeros(lay8.total, dtype=torch.float32, device="cuda")
    hp.build_hzb(to_device(g8.depth), hzb8, lay8)
    del g8
    consts = hostmath.pack_culling_constants(fc8.view, fc8.proj, n, True, lay8.count, lay8.width, lay8.height, False)
    bounds = to_device(synth.instances_random(n, synth.SEED_BASE + 5, center=fc8.camera_position, box=400.0))
    args0 = to_device(synth.indirect_args_initial(n))
    sets = [dict(bounds=bounds if k == 0 else bounds.clone(), args=args0.clone(), vis=torch.zeros(n, dtype=torch.int32, device="cuda"),
                 cmds=torch.zeros(n * 16, dtype=torch.int32, device="cuda")) for k in range(a.ring)]
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    rng = np.random.default_rng(4096)
    layouts = {"none": None, "R=1": np.array([0, n], np.uint32), "R=64": np.linspace(0, n, 65).astype(np.uint32),
               "R=4096": np.sort(np.concatenate([[0], rng.integers(0, n + 1, 4095), [n]])).astype(np.uint32),
               "R=n": np.arange(n + 1, dtype=np.uint32)}
    dev_layouts = {k: None if o is None else (hp.draw_offsets_to_device(o, n), torch.zeros(o.size - 1, dtype=torch.int32, device="cuda"))
                   for k, o in layouts.items()}
    turn = [0]

    def call(key):
        s = sets[turn[0] % a.ring]
        turn[0] += 1
        d = dev_layouts[key]
        if d is None:
            hp.cull_indirect_args(consts, s["bounds"], hzb8, lay8, s["args"], None, s["vis"], cnt)
        else:
            hp.cull_indirect_args(consts, s["bounds"], hzb8, lay8, s["args"], None, s["vis"], cnt, draw_offsets=d[0], draw_commands=s["cmds"],
                                  draw_counts=d[1])

    for key in layouts:  # warm-up, and the steady state of the words (UR_OPT_CULL_STORE = 3) in every set
        for _ in range(a.ring):
            call(key)
    torch.cuda.synchronize()
    visible = int(cnt.cpu()[0])
    times = {k: [] for k in layouts}
    for _ in range(a.batches):
        for key in layouts:
            times[key].append(time_batch(torch, lambda k, key=key: call(key), a.iters))
    rows = []
    for key, t in times.items():
        rows.append({"shape": f"C5 {n} instances, {visible} visible, list on, ranges {key}", "median_us": float(np.median(t)),
                     "min_us": float(np.min(t)), "batches": len(t), "calls_per_batch": a.iters, "inputs": f"{a.ring} buffer sets cycled (cold)"})
    del sets, dev_layouts
    torch.cuda.empty_cache()

    # the single-block calls: the scenes' own command AABBs and cameras
    for name, file in (("sponza", "sponza"), ("pica_pica", "pica_pica")):
        sb = scene.load_scene_bounds(ROOT / "tests" / "golden" / "assets" / "Scenes" / f"{file}.json")
        m = sb.count
        fc = hostmath.build_frame_constants(name, 1920, 1080)
        lay = HzbLayout(1920, 1080)
        g = synth.gbuffer_scene(fc.view, fc.proj, fc.camera_position, 1920, 1080, 7)
        hzb = torch.zeros(lay.total, dtype=torch.float32, device="cuda")
        hp.build_hzb(to_device(g.depth), hzb, lay)
        c = hostmath.pack_culling_constants(fc.view, fc.proj, m, True, lay.count, lay.width, lay.height, False)
        d_b, d_a = to_device(sb.bounds), to_device(synth.indirect_args_initial(m))
        d_v, d_c = torch.zeros(m, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
        d_cmds, d_counts = torch.zeros(m * 16, dtype=torch.int32, device="cuda"), torch.zeros(m, dtype=torch.int32, device="cuda")
        d_o = hp.draw_offsets_to_device(scene.draw_offsets(np.arange(m)), m)
        plain = lambda k: hp.cull_indirect_args(c, d_b, hzb, lay, d_a, None, d_v, d_c)
        ranged = lambda k: hp.cull_indirect_args(c, d_b, hzb, lay, d_a, None, d_v, d_c, draw_offsets=d_o, draw_commands=d_cmds, draw_counts=d_counts)
        for f in (plain, ranged):
            for k in range(5):
                f(k)
        torch.cuda.synchronize()
        tp, tr = [], []
        for _ in range(a.batches):
            tp.append(time_batch(torch, plain, a.iters * 4))
            tr.append(time_batch(torch, ranged, a.iters * 4))
        for key, t in (("none", tp), ("one per command", tr)):
            rows.append({"shape": f"{name} {m} commands, list on, ranges {key}", "median_us": float(np.median(t)), "min_us": float(np.min(t)),
                         "batches": len(t), "calls_per_batch": a.iters * 4, "inputs": "one buffer set"})
    hp.close()
    for r in rows:
        print(f"{r['shape']:70s} median {r['median_us']:8.2f} us  min {r['min_us']:8.2f} us")
    if a.json:
        with open(a.json, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    print(json.dumps({"tool": "bench_cull_draws", "quick": a.quick, "results": rows}))


if __name__ == "__main__":
    main()
