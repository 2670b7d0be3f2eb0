#!/usr/bin/env python3
"""Timing of the cull with draw ranges (ur_cull_indirect_args_draws) and with extra views (ur_cull_indirect_args_views) on one GPU
(development aid; bench.py is the contract benchmark and never sets ranges or views).

    python tools/bench_cull.py [--shapes ranges|views|both] [--batches 9] [--iters 30] [--json out.jsonl]
    python tools/bench_cull.py --quick      # each shape a few times: for a rocprofv3 --kernel-trace --stats run

C5 (BASELINE config 5): 1 M instance AABBs against the 12-mip HZB of a 7680x4320 depth, with the camera's visible list, over six
rotating buffer sets (bounds, commands, lists, masks and compacted commands: cold, as bench.py's extras). The plain call, then
  ranges: R = 1, 64, 4096 (a random partition) and one range per command;
  views:  one view (mask; mask + list; R = 64 ranges), two and four views (masks), and the two-call alternative - the plain call,
          then ur_cull_indirect_args with the light's constants and HZBEnabled = 0 into a second command buffer.
The shapes alternate batch by batch in one process. Then the single-block calls of Sponza's 25 and pica_pica's 170 commands: plain,
with one range per command (ranges) and with one view (views). Each time is one device-event pair around a batch of back-to-back
calls, divided by the calls (launch gaps included). Kernel times and launch counts come from a separate rocprofv3 --kernel-trace
--stats run of --quick.
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
    ap.add_argument("--shapes", choices=("ranges", "views", "both"), default="both", help="the shapes beside the plain call")
    ap.add_argument("--instances", type=int, default=1_000_000)
    ap.add_argument("--batches", type=int, default=9)
    ap.add_argument("--iters", type=int, default=30, help="calls per timed batch")
    ap.add_argument("--ring", type=int, default=6, help="buffer sets cycled through so that every call meets cold inputs")
    ap.add_argument("--quick", action="store_true", help="each shape a few times (for the profiler run)")
    ap.add_argument("--json", default="", help="also append one JSON line per shape to this file")
    a = ap.parse_args()
    if a.quick:
        a.batches, a.iters, a.ring = 1, 3, 2
    ranges, views = a.shapes in ("ranges", "both"), a.shapes in ("views", "both")
    import torch
    from unclerenderer_amd import hostmath, scene, synth
    from unclerenderer_amd.hotpath import HotPath, HzbLayout, cull_view, to_device
    assert torch.cuda.is_available(), "bench_cull needs a GPU"
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
    light_vp = hostmath.light_view_projection(fc8.scene_center, fc8.scene_radius, fc8.light_direction)
    light = hostmath.frustum_planes(light_vp)
    cascade = hostmath.frustum_planes(hostmath.light_view_projection(fc8.scene_center, fc8.scene_radius * 0.25, fc8.light_direction))
    cam = np.ascontiguousarray(consts[:24]).view(np.float32).copy()
    planes = [light, cam, cascade, light]
    # the second call of the two-call alternative: the light's view-projection as the camera, no HZB
    light_consts = hostmath.pack_culling_constants(np.eye(4, dtype=np.float32).reshape(-1), light_vp, n, False, 0, 0, 0, False)
    light_consts[:24] = light.view(np.uint32)
    bounds = to_device(synth.instances_random(n, synth.SEED_BASE + 5, center=fc8.camera_position, box=400.0))
    args0 = to_device(synth.indirect_args_initial(n))
    words = (n + 31) // 32
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    rng = np.random.default_rng(4096)
    layouts = {"R=1": np.array([0, n], np.uint32), "R=64": np.linspace(0, n, 65).astype(np.uint32),
               "R=4096": np.sort(np.concatenate([[0], rng.integers(0, n + 1, 4095), [n]])).astype(np.uint32),
               "R=n": np.arange(n + 1, dtype=np.uint32)}
    dev_layouts = {k: (hp.draw_offsets_to_device(o, n), torch.zeros(o.size - 1, dtype=torch.int32, device="cuda")) for k, o in layouts.items()}
    zeros = lambda k: torch.zeros(k, dtype=torch.int32, device="cuda")
    sets = []
    for k in range(a.ring):
        s = dict(bounds=bounds if k == 0 else bounds.clone(), args=args0.clone(), vis=zeros(n), cmds=zeros(n * 16))
        if views:
            s.update(args2=args0.clone(), masks=[zeros(words) for _ in range(4)], vvis=zeros(n), vcnt=zeros(1), vcounts=zeros(64))
        sets.append(s)
    # shape -> the keyword arguments of the call on buffer set s (None: the two-call alternative)
    shapes = {"plain": lambda s: {}}
    if ranges:
        for key, (d_o, d_n) in dev_layouts.items():
            shapes[f"ranges {key}"] = lambda s, d_o=d_o, d_n=d_n: dict(draw_offsets=d_o, draw_commands=s["cmds"], draw_counts=d_n)
    if views:
        d_o64 = dev_layouts["R=64"][0]
        shapes.update({
            "1 view, mask": lambda s: dict(views=[cull_view(light, mask=s["masks"][0])]),
            "1 view, mask + list": lambda s: dict(views=[cull_view(light, mask=s["masks"][0], visible_idx=s["vvis"], visible_count=s["vcnt"])]),
            "1 view, R=64 ranges": lambda s: dict(views=[cull_view(light, draw_offsets=d_o64, draw_commands=s["cmds"], draw_counts=s["vcounts"])]),
            "2 views, masks": lambda s: dict(views=[cull_view(planes[i], mask=s["masks"][i]) for i in range(2)]),
            "4 views, masks": lambda s: dict(views=[cull_view(planes[i], mask=s["masks"][i]) for i in range(4)]),
            "two calls (plain + light, HZB off)": None,
        })
    calls = {key: [f(s) if f is not None else None for s in sets] for key, f in shapes.items()}  # (built once per buffer set)
    turn = [0]

    def call(key):
        i = turn[0] % a.ring
        s, kw = sets[i], calls[key][i]
        turn[0] += 1
        hp.cull_indirect_args(consts, s["bounds"], hzb8, lay8, s["args"], None, s["vis"], cnt, **(kw or {}))
        if kw is None:
            hp.cull_indirect_args(light_consts, s["bounds"], None, None, s["args2"], None)

    for key in shapes:  # warm-up, and the steady state of the words (UR_OPT_CULL_STORE = 3) in every set
        for _ in range(a.ring):
            call(key)
    torch.cuda.synchronize()
    visible = int(cnt.cpu()[0])
    times = {k: [] for k in shapes}
    for _ in range(a.batches):
        for key in shapes:
            times[key].append(time_batch(torch, lambda k, key=key: call(key), a.iters))
    rows = []
    for key, t in times.items():
        rows.append({"shape": f"C5 {n} instances, {visible} visible, list on, {key}", "median_us": float(np.median(t)),
                     "min_us": float(np.min(t)), "max_us": float(np.max(t)), "batches": len(t), "calls_per_batch": a.iters,
                     "inputs": f"{a.ring} buffer sets cycled (cold)"})
    del sets, calls, dev_layouts
    torch.cuda.empty_cache()

    # the single-block calls: the scenes' own command AABBs and cameras
    for name in ("sponza", "pica_pica"):
        sb = scene.load_scene_bounds(ROOT / "tests" / "golden" / "assets" / "Scenes" / f"{name}.json")
        m = sb.count
        fc = hostmath.build_frame_constants(name, 1920, 1080)
        lay = HzbLayout(1920, 1080)
        g = synth.gbuffer_scene(fc.view, fc.proj, fc.camera_position, 1920, 1080, 7)
        hzb = torch.zeros(lay.total, dtype=torch.float32, device="cuda")
        hp.build_hzb(to_device(g.depth), hzb, lay)
        c = hostmath.pack_culling_constants(fc.view, fc.proj, m, True, lay.count, lay.width, lay.height, False)
        d_b, d_a = to_device(sb.bounds), to_device(synth.indirect_args_initial(m))
        d_v, d_c = zeros(m), zeros(1)
        small = {"plain": {}}
        if ranges:
            small["ranges one per command"] = dict(draw_offsets=hp.draw_offsets_to_device(scene.draw_offsets(np.arange(m)), m),
                                                  draw_commands=zeros(m * 16), draw_counts=zeros(m))
        if views:
            lv = hostmath.frustum_planes(hostmath.light_view_projection(fc.scene_center, fc.scene_radius, fc.light_direction))
            small["1 view, mask"] = dict(views=[cull_view(lv, mask=zeros((m + 31) // 32))])
        fns = {key: lambda k, kw=kw: hp.cull_indirect_args(c, d_b, hzb, lay, d_a, None, d_v, d_c, **kw) for key, kw in small.items()}
        for f in fns.values():
            for k in range(5):
                f(k)
        torch.cuda.synchronize()
        ts = {key: [] for key in fns}
        for _ in range(a.batches):
            for key, f in fns.items():
                ts[key].append(time_batch(torch, f, a.iters * 4))
        for key, t in ts.items():
            rows.append({"shape": f"{name} {m} commands, list on, {key}", "median_us": float(np.median(t)), "min_us": float(np.min(t)),
                         "max_us": float(np.max(t)), "batches": len(t), "calls_per_batch": a.iters * 4, "inputs": "one buffer set"})
    hp.close()
    for r in rows:
        print(f"{r['shape']:80s} median {r['median_us']:8.2f} us  min {r['min_us']:8.2f} us")
    if a.json:
        with open(a.json, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    print(json.dumps({"tool": "bench_cull", "shapes": a.shapes, "quick": a.quick, "results": rows}))


if __name__ == "__main__":
    main()
