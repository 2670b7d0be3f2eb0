#!/usr/bin/env python3
"""Timing of the cull with extra views (ur_cull_indirect_args_views) on one GPU (development aid; bench.py is the contract benchmark
and never sets views).

    python tools/bench_cull_views.py [--batches 9] [--iters 30] [--json out.jsonl]
    python tools/bench_cull_views.py --quick      # each shape a few times: for a rocprofv3 --kernel-trace --stats run

C5 (BASELINE config 5): 1 M instance AABBs against the 12-mip HZB of a 7680x4320 depth, with the camera's visible list, over six
rotating buffer sets (cold, as bench.py's extras): the plain call, plus one view (mask; mask + list; R = 64 ranges), plus two and four
views (masks), and the two-call alternative - the plain call, then ur_cull_indirect_args with the light's constants and HZBEnabled = 0
into a second command buffer. The shapes alternate batch by batch in one process. Then the single-block calls of Sponza's 25 and
pica_pica's 170 commands with and without one view. Each time is one device-event pair around a batch of back-to-back calls, divided
by the calls (launch gaps included). Kernel times and launch counts come from a separate rocprofv3 --kernel-trace --stats run of --quick.
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
    from unclerenderer_amd.hotpath import HotPath, HzbLayout, cull_view, to_device
    assert torch.cuda.is_available(), "bench_cull_views needs a GPU"
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
    o64 = np.linspace(0, n, 65).astype(np.uint32)
    d_o64 = hp.draw_offsets_to_device(o64, n)
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    sets = []
    for k in range(a.ring):
        s = dict(bounds=bounds if k == 0 else bounds.clone(), args=args0.clone(), vis=torch.zeros(n, dtype=torch.int32, device="cuda"),
                 args2=args0.clone(), masks=[torch.zeros(words, dtype=torch.int32, device="cuda") for _ in range(4)],
                 vvis=torch.zeros(n, dtype=torch.int32, device="cuda"), vcnt=torch.zeros(1, dtype=torch.int32, device="cuda"),
                 cmds=torch.zeros(n * 16, dtype=torch.int32, device="cuda"), counts=torch.zeros(64, dtype=torch.int32, device="cuda"))
        s["views"] = {
            "none": None,
            "1 view, mask": [cull_view(light, mask=s["masks"][0])],
            "1 view, mask + list": [cull_view(light, mask=s["masks"][0], visible_idx=s["vvis"], visible_count=s["vcnt"])],
            "1 view, R=64 ranges": [cull_view(light, draw_offsets=d_o64, draw_commands=s["cmds"], draw_counts=s["counts"])],
            "2 views, masks": [cull_view(planes[i], mask=s["masks"][i]) for i in range(2)],
            "4 views, masks": [cull_view(planes[i], mask=s["masks"][i]) for i in range(4)],
        }
        sets.append(s)
    shapes = list(sets[0]["views"]) + ["two calls (plain + light, HZB off)"]
    turn = [0]

    def call(key):
        s = sets[turn[0] % a.ring]
        turn[0] += 1
        if key.startswith("two calls"):
            hp.cull_indirect_args(consts, s["bounds"], hzb8, lay8, s["args"], None, s["vis"], cnt)
            hp.cull_indirect_args(light_consts, s["bounds"], None, None, s["args2"], None)
        else:
            hp.cull_indirect_args(consts, s["bounds"], hzb8, lay8, s["args"], None, s["vis"], cnt, views=s["views"][key])

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
                     "min_us": float(np.min(t)), "batches": len(t), "calls_per_batch": a.iters, "inputs": f"{a.ring} buffer sets cycled (cold)"})
    del sets
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
        d_v, d_c = torch.zeros(m, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
        d_m = torch.zeros((m + 31) // 32, dtype=torch.int32, device="cuda")
        lv = [cull_view(hostmath.frustum_planes(hostmath.light_view_projection(fc.scene_center, fc.scene_radius, fc.light_direction)), mask=d_m)]
        plain = lambda k: hp.cull_indirect_args(c, d_b, hzb, lay, d_a, None, d_v, d_c)
        viewed = lambda k: hp.cull_indirect_args(c, d_b, hzb, lay, d_a, None, d_v, d_c, views=lv)
        for f in (plain, viewed):
            for k in range(5):
                f(k)
        torch.cuda.synchronize()
        tp, tv = [], []
        for _ in range(a.batches):
            tp.append(time_batch(torch, plain, a.iters * 4))
            tv.append(time_batch(torch, viewed, a.iters * 4))
        for key, t in (("no view", tp), ("1 view, mask", tv)):
            rows.append({"shape": f"{name} {m} commands, list on, {key}", "median_us": float(np.median(t)), "min_us": float(np.min(t)),
                         "batches": len(t), "calls_per_batch": a.iters * 4, "inputs": "one buffer set"})
    hp.close()
    for r in rows:
        print(f"{r['shape']:80s} median {r['median_us']:8.2f} us  min {r['min_us']:8.2f} us")
    if a.json:
        with open(a.json, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    print(json.dumps({"tool": "bench_cull_views", "quick": a.quick, "results": rows}))


if __name__ == "__main__":
    main()
