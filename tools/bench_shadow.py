#!/usr/bin/env python3
"""Timing of the ShadowMap pass (ur_shadow_map) on one GPU (development aid; bench.py is the contract benchmark and never draws).

    python tools/bench_shadow.py [--batches 7] [--iters 10] [--json out.jsonl]
    python tools/bench_shadow.py --quick     # each workload a few times: for a rocprofv3 --kernel-trace --stats run
    python tools/bench_shadow.py --pass both # ShadowMap, then the DepthPrepass pass (ur_depth_prepass) over the same triangles
    python tools/bench_shadow.py --pass gbuffer # the GBuffer pass (ur_gbuffer_pass) at 3840 x 2160, its two halves timed apart
    python tools/bench_shadow.py --pass gbuffer --textured # the textured resolve (key 15) beside the untextured one and a streaming kernel
    python tools/bench_shadow.py --pass gbuffer --textured --bc 1 # the same with the four maps as BC1 blocks (--bc 3, --bc 5; --pass forward too)
    python tools/bench_shadow.py --pass gbuffer --masked # the alpha-masked raster (ur_gbuffer_pass_masked) beside the all-opaque one
    python tools/bench_shadow.py --pass forward [--textured] [--masked] # the forward resolve beside the GBuffer resolve + ur_deferred_lighting

A 2048 x 2048 map over three workloads, each with and without a large-triangle queue (ur_raster_reserve):
  small   1 M triangles of 1/8 px to 8 px in one command;
  large   a soup of 256 map-spanning triangles;
  mix     the two together, as two commands.
Each time is one device-event pair around a batch of back-to-back calls over rotating buffer sets (cold maps), divided by the calls
(launch gaps included). Beside them, measured in the same run, the yardstick that exists today: the clear alone (a call with no
commands launches only the clear: 16.8 MB of stores). The per-launch split (clear / raster / large) comes from a separate rocprofv3
--kernel-trace --stats run of --quick: the kernels are shadow_clear_kernel, raster_kernel<ShadowPolicy> and large_kernel<ShadowPolicy>
(<DepthPolicy<...>> for the prepass). The second yardstick of the plan - a plain kernel issuing the same number of contiguous
atomic-minimum bytes - needs a fragment count the pass does not keep and is not built.

The depth leg draws the same triangles under a perspective camera: a vertex at clip (x, y, z) becomes the view-space position
(x * v, y * v, v) with v = NEAR / z, under View = identity and the projection clip = (x, y, NEAR, w = view z), its triangle's winding
reversed (the prepass draws the other facing). It lands on the same pixel up to the rounding of x * v / v, with the same depth order
reversed (reverse-Z): the same fragments, a maximum instead of a minimum, plus the three products, the near-plane test and the divides.

The gbuffer leg draws the small and the large workload, scaled to a 3840 x 2160 target, as the depth leg draws them, with 64-byte
vertices (a unit normal, a seeded colour) and a whole constant block. Per workload every buffer set of the ring first gets its depth
from ur_depth_prepass and its keys from the raster part; then, batch by batch in the same process, four times are taken over the ring:
ur_depth_prepass on this input (the yardstick of clear + raster: what the pass adds is the depth load and compare, and the atomic on the
key image), the clear + raster (+ queue) launches alone and the resolve launch alone (ur_gbuffer_pass_parts), and the whole pass. Beside
the resolve, two yardsticks for its 4 B key + 28 B targets per texel (+4 with ObjectId): the resolve of an empty key image (a call
without commands: the same loads and stores, no triangle), and the plain streaming kernel (ur_debug_stream_ceiling: four reads to one
write) moving the same byte count.
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
SIZE = 2048
GBUFFER_W, GBUFFER_H = 3840, 2160


def time_batch(torch, fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for k in range(iters):
        fn(k)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def triangles(rng, n, lo, hi, w=SIZE, h=SIZE):
    """n clockwise-on-target triangles (drawn) with edge lengths log-uniform in [lo, hi] px, as clip-space positions (n * 3, 3)."""
    c = rng.uniform(0, (w, h), (n, 1, 2))
    length = np.exp(rng.uniform(np.log(lo), np.log(hi), (n, 1, 1)))
    p = c + rng.uniform(-0.5, 0.5, (n, 3, 2)) * length
    e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    flip = e1[:, 0] * e2[:, 1] - e2[:, 0] * e1[:, 1] < 0
    p[flip] = p[flip][:, [0, 2, 1]]
    z = rng.uniform(0.05, 0.95, (n, 3, 1))
    return np.concatenate([p[..., :1] / (0.5 * w) - 1.0, 1.0 - p[..., 1:] / (0.5 * h), z], axis=2).reshape(-1, 3).astype(np.float32)


NEAR = 0.125
VIEW = np.eye(4, dtype=np.float32).reshape(-1)
PROJ = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, NEAR, 0], np.float32)


def camera_space(pos):
    v = NEAR / pos[:, 2:3].astype(np.float64)
    p = np.concatenate([pos[:, :2] * v, v], axis=1).astype(np.float32)
    return p.reshape(-1, 3, 3)[:, [0, 2, 1]].reshape(-1, 3)


def gbuffer_leg(a, torch, hp):
    """The rows of --pass gbuffer (the module's docstring says what is timed against what)."""
    from unclerenderer_amd import lib
    from unclerenderer_amd.hotpath import gbuffer_targets, pack_draw_commands, to_device
    w, h = GBUFFER_W, GBUFFER_H
    rng = np.random.default_rng(2160)
    cb = np.zeros(152, np.float32)  # ur_scene_constants: World, BaseColor at float 64, EmissiveFactor at 80, Metallic / Roughness at 104 / 105, ObjectId at 148
    cb[:16] = np.eye(4, dtype=np.float32).reshape(-1)
    cb[64:68], cb[80:83], cb[104], cb[105] = (0.8, 0.7, 0.6, 1.0), (0.1, 0.2, 0.3), 0.25, 0.5
    cb.view(np.uint32)[148] = 7
    constants = to_device(cb)

    def mesh(pos):
        v = np.zeros((pos.shape[0], 16), np.float32)
        v[:, :3], v[:, 5] = pos, -1.0
        v[:, 12:15], v[:, 15] = rng.uniform(0.0, 1.0, (pos.shape[0], 3)), 1.0
        return dict(vertices=to_device(v.reshape(-1)), indices=to_device(np.arange(pos.shape[0], dtype=np.uint32)), constants=constants, stride=64)

    loads = {"small": mesh(camera_space(triangles(rng, a.small, 0.125, 8.0, w, h))), "large": mesh(camera_space(triangles(rng, 256, w, 2 * w, w, h)))}
    cmds = {k: to_device(pack_draw_commands([v])) for k, v in loads.items()}
    half = lambda: torch.empty((h, w, 4), dtype=torch.float16, device="cuda")  # noqa: E731
    word = lambda: torch.zeros((h, w), dtype=torch.int32, device="cuda")  # noqa: E731
    sets = []
    for _ in range(a.ring):
        ga, gb, hdr, gc, keys, oid = half(), half(), half(), word(), word(), word()
        sets.append((torch.zeros((h, w), dtype=torch.float32, device="cuda"), gbuffer_targets(ga, gb, gc, hdr, keys), gbuffer_targets(ga, gb, gc, hdr, keys, oid)))
    stats = torch.zeros(6, dtype=torch.int32, device="cuda")
    RASTER, RESOLVE = lib.UR_GBUFFER_PART_RASTER, lib.UR_GBUFFER_PART_RESOLVE

    def stream(nbytes):
        n16 = nbytes // (5 * 16)
        gen = torch.Generator(device="cuda")
        gen.manual_seed(1234)
        ring = [([(torch.randint(0, 0x3FFF, (n16 * 8,), dtype=torch.int16, device="cuda", generator=gen) | 0x3000) for _ in range(4)],
                 torch.empty(n16 * 8, dtype=torch.int16, device="cuda")) for _ in range(a.ring)]
        fn = lambda i: hp.stream_ceiling(*ring[i % a.ring])  # noqa: E731
        fn(0)
        torch.cuda.synchronize()
        return [time_batch(torch, fn, a.iters) for _ in range(a.batches)]

    rows = []

    def row(shape, t, seen=None, **more):
        rows.append({"shape": f"{w}x{h}, gbuffer, {shape}", "median_us": float(np.median(t)), "min_us": float(np.min(t)), "max_us": float(np.max(t)), "stats_one_call": seen or [],
                     "batches": len(t), "calls_per_batch": a.iters, "maps": a.ring, **more})

    for oid in (False, True):
        nbytes = (36 if oid else 32) * w * h
        row(f"streaming kernel of {nbytes} B (4 reads : 1 write), the resolve's bytes {'with' if oid else 'without'} ObjectId", stream(nbytes), bytes=nbytes)
    for reserve in (a.reserve, 0):
        hp.raster_reserve(reserve)
        for name, c in {"no commands": None, **cmds}.items():
            count = None if c is not None else 0
            gb = lambda i, parts, oid=False, st=None: hp.gbuffer_pass(VIEW, PROJ, c, sets[i % a.ring][0], sets[i % a.ring][2 if oid else 1], w, h,  # noqa: E731
                                                                      stats=st, command_count=count, parts=parts)
            prepass = lambda i, st=None: hp.depth_prepass(VIEW, PROJ, c, sets[i % a.ring][0], stats=st, command_count=count)  # noqa: E731
            # every set of the ring: the depth of these draws, and their keys (the resolve part reads the keys as they are: never another workload's)
            for i in range(a.ring):
                prepass(i)
                gb(i, RASTER)
            stats.zero_()
            gb(0, RASTER, st=stats if c is not None else None)
            torch.cuda.synchronize()
            seen = stats.cpu().numpy().view(np.uint32).tolist()
            drawn = int((sets[0][1]._keep[4] != 0).sum())
            fns = {"DepthPrepass on this input": prepass, "clear + raster": lambda i: gb(i, RASTER), "resolve": lambda i: gb(i, RESOLVE),
                   "resolve with ObjectId": lambda i: gb(i, RESOLVE, True), "whole pass": lambda i: gb(i, RASTER | RESOLVE)}
            times = {k: [] for k in fns}
            for _ in range(a.batches):
                for k, f in fns.items():
                    times[k].append(time_batch(torch, f, a.iters))
            for k, t in times.items():
                row(f"{name}, reserve {reserve}, {k}", t, seen, texels_drawn=drawn)
    return rows


BC_FORMATS = {1: (71, 72), 3: (77, 78), 5: (83, 83)}  # --bc N: (UR_TEXTURE_BCN_UNORM, its _SRGB form; BC5 has none)


def bc_chain_1024(rng, bc: int, srgb: bool):
    """A full 1024 x 1024 chain of random blocks (every bit pattern is a valid block): (blocks, format, the decoded levels for the host-side
    probe count, by ur_host_bc_decode_level)."""
    from unclerenderer_amd import hostmath
    fmt = BC_FORMATS[bc][1 if srgb else 0]
    data = rng.integers(0, 256, hostmath.bc_chain_bytes(fmt, 1024, 1024, 11), dtype=np.uint8)
    levels, at = [], 0
    for k in range(11):
        size = max(1, 1024 >> k)
        levels.append(hostmath.bc_decode_level(fmt, data[at:], size, size))
        at += hostmath.bc_chain_bytes(fmt, size, size, 1)
    return data, fmt, levels


def gbuffer_textured_leg(a, torch, hp):
    """The rows of --pass gbuffer --textured: at 3840 x 2160 over cold buffer sets, the resolve part alone (ur_gbuffer_pass_materials_parts)
    with the one command on pipeline key 15 - two 1024 x 1024 sRGB (base colour, emissive) and two UNORM (metallic-roughness, normal)
    textures with full chains of random bytes -, interleaved in the same process with the untextured resolve over the same keys (the
    yardstick) and the streaming kernel of the resolve's 32 bytes per texel. TEXCOORD is the target position / 256 px in u and 2.5 x
    that in v: about 4 x 10 texels per pixel, so the nominal footprint is N = 3 probes between levels 2 and 3 (the perspective of each
    triangle moves it a little; the mean probe count of a row is computed on the host by the numpy restatement over every 64th texel of the
    keys the device rasterised). Only the targets are ringed: the four 5.6 MB texture chains are shared by every set of the ring, so
    they stay warm in the L2 and the Infinity Cache, as a frame's textures would between passes but not as a streamed scene's would.
    --bc N: the same four chains as random BC1 / BC3 / BC5 blocks (1.4 MB each in BC3 and BC5, half that in BC1), sRGB forms where RGBA8's are."""
    from unclerenderer_amd import lib
    from unclerenderer_amd.hotpath import gbuffer_targets, pack_draw_commands, pack_materials, pack_texture, pack_texture_bc, to_device
    w, h = GBUFFER_W, GBUFFER_H
    rng = np.random.default_rng(2161)
    cb = np.zeros(152, np.float32)
    cb[:16] = np.eye(4, dtype=np.float32).reshape(-1)
    cb[64:68], cb[80:83], cb[104], cb[105] = (0.8, 0.7, 0.6, 1.0), (0.1, 0.2, 0.3), 0.25, 0.5
    for at in (112, 120, 128, 136):  # the four texture transforms: identity
        cb[at + 2], cb[at + 3], cb[at + 4] = 1.0, 1.0, 1.0
    constants = to_device(cb)

    def mesh(pos):
        v = np.zeros((pos.shape[0], 16), np.float32)
        v[:, :3], v[:, 5] = pos, -1.0
        v[:, 6] = pos[:, 0] / pos[:, 2] * (0.5 * w / 256.0)
        v[:, 7] = pos[:, 1] / pos[:, 2] * (0.5 * h / 256.0 * 2.5)
        v[:, 8], v[:, 11] = 1.0, 1.0
        v[:, 12:15], v[:, 15] = rng.uniform(0.0, 1.0, (pos.shape[0], 3)), 1.0
        return dict(vertices=to_device(v.reshape(-1)), indices=to_device(np.arange(pos.shape[0], dtype=np.uint32)), constants=constants, stride=64)

    chain = lambda: [rng.integers(0, 256, (max(1, 1024 >> k), max(1, 1024 >> k), 4), dtype=np.uint8) for k in range(11)]  # noqa: E731
    srgb_of = {"base_color": True, "emissive": True, "metallic_roughness": False, "normal": False}
    if a.bc:
        blocks = {k: bc_chain_1024(rng, a.bc, srgb) for k, srgb in srgb_of.items()}
        chains = {k: (levels, fmt in (72, 78)) for k, (_, fmt, levels) in blocks.items()}  # the decoded twins, for mean_probes
        materials = pack_materials([{"key": 15, **{k: pack_texture_bc(data, 1024, 1024, 11, fmt) for k, (data, fmt, _) in blocks.items()}}])
    else:
        chains = {k: (chain(), srgb) for k, srgb in srgb_of.items()}
        materials = pack_materials([{"key": 15, **{k: pack_texture(*v) for k, v in chains.items()}}])
    maps_label = f"four 1024 x 1024 BC{a.bc} maps" if a.bc else "four 1024 x 1024 maps"
    host_vertices = {}

    def mesh_kept(name, pos):
        m = mesh(pos)
        host_vertices[name] = m["vertices"].cpu().numpy().view(np.uint8)
        return m

    def mean_probes(name, keys):
        """The mean probe count per sampled map of every 8th texel of every 8th row, by the numpy restatement (tests/gbuffer_tex_ref.py)
        on the keys the device rasterised: the restatement is byte-equal to the kernel, so these are the kernel's probe counts."""
        from tests import gbuffer_tex_ref as X
        sampled = np.zeros_like(keys)
        sampled[::8, ::8] = keys[::8, ::8]
        v = host_vertices[name]
        d = X.TexDraw(v, np.arange(v.size // 64, dtype=np.uint32))
        g = X.gather([d], VIEW, PROJ, sampled, w, h, {0: 0}, X.G.key_bits(1))
        r = X.shade(g, VIEW, [{"key": 15, **{k: X.Tex(lv, srgb) for k, (lv, srgb) in chains.items()}}])
        n = np.concatenate([N for runs in r["info"].values() for (_, N, _, _, _) in runs])
        lod = np.concatenate([L for runs in r["info"].values() for (_, _, L, _, _) in runs])
        return float(n.mean()), float(lod.mean()) / 256.0, int(g["at"].size)

    loads = {"small": mesh_kept("small", camera_space(triangles(rng, a.small, 0.125, 8.0, w, h))),
             "large": mesh_kept("large", camera_space(triangles(rng, 256, w, 2 * w, w, h)))}
    cmds = {k: to_device(pack_draw_commands([v])) for k, v in loads.items()}
    sets = []
    for _ in range(a.ring):
        ga, gb, hdr = (torch.empty((h, w, 4), dtype=torch.float16, device="cuda") for _ in range(3))
        gc, keys = (torch.zeros((h, w), dtype=torch.int32, device="cuda") for _ in range(2))
        sets.append((torch.zeros((h, w), dtype=torch.float32, device="cuda"), gbuffer_targets(ga, gb, gc, hdr, keys)))
    RASTER, RESOLVE = lib.UR_GBUFFER_PART_RASTER, lib.UR_GBUFFER_PART_RESOLVE
    n16 = (32 * w * h) // (5 * 16)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1234)
    ring = [([(torch.randint(0, 0x3FFF, (n16 * 8,), dtype=torch.int16, device="cuda", generator=gen) | 0x3000) for _ in range(4)],
             torch.empty(n16 * 8, dtype=torch.int16, device="cuda")) for _ in range(a.ring)]
    rows = []
    hp.raster_reserve(a.reserve)
    for name, c in cmds.items():
        gb = lambda i, parts, m=None: hp.gbuffer_pass(VIEW, PROJ, c, sets[i % a.ring][0], sets[i % a.ring][1], w, h, parts=parts, materials=m)  # noqa: E731
        for i in range(a.ring):
            hp.depth_prepass(VIEW, PROJ, c, sets[i][0])
            gb(i, RASTER)
        torch.cuda.synchronize()
        drawn = int((sets[0][1]._keep[4] != 0).sum())
        probes, level, sampled = mean_probes(name, sets[0][1]._keep[4].cpu().numpy().view(np.uint32)) if not a.no_probe_count else (None, None, 0)
        fns = {"streaming kernel of the resolve's 32 B per texel": lambda i: hp.stream_ceiling(*ring[i % a.ring]),
               "resolve, untextured": lambda i: gb(i, RESOLVE), f"resolve, key 15 ({maps_label})": lambda i: gb(i, RESOLVE, materials)}
        times = {k: [] for k in fns}
        for f in fns.values():
            f(0)
        torch.cuda.synchronize()
        for _ in range(a.batches):
            for k, f in fns.items():
                times[k].append(time_batch(torch, f, a.iters))
        base = float(np.median(times["resolve, untextured"]))
        for k, t in times.items():
            rows.append({"shape": f"{w}x{h}, gbuffer textured, {name}, {k}", "median_us": float(np.median(t)), "min_us": float(np.min(t)), "max_us": float(np.max(t)), "stats_one_call": [],
                         "batches": len(t), "calls_per_batch": a.iters, "maps": a.ring, "texels_drawn": drawn, "ratio_to_untextured": float(np.median(t)) / base,
                         "mean_probes_per_map": probes, "mean_level": level, "texels_sampled_for_probes": sampled})
    return rows


def gbuffer_masked_leg(a, torch, hp):
    """The rows of --pass gbuffer --masked: at 3840 x 2160 over cold buffer sets, the textured small-triangle workload cut into 8 commands
    on one 1024 x 1024 base-colour map whose alpha is random bytes; 3 of the 8 (slots 2, 5, 7) are the masked selection on pipeline key
    31, the others the opaque one on key 15. ur_gbuffer_pass_masked raises the depth it is given, so every timed call starts with the
    DepthPrepass it belongs behind, and the prepasses are timed alone beside them, in the same process, batch by batch:
      DepthPrepass of the opaque draws;              ... + the raster part with the mask (six raster launches and the merge);
      DepthPrepass of all draws;                     ... + the raster part of ur_gbuffer_pass_materials on all draws, bit 4 cleared;
                                                     ... + the whole ur_gbuffer_pass_materials on all draws, bit 4 cleared;
      DepthPrepass of the opaque draws + the whole ur_gbuffer_pass_masked.
    stats_one_call of a masked row is the masked draws' stats6; `won` the texels a masked fragment won in one call."""
    from unclerenderer_amd import lib
    from unclerenderer_amd.hotpath import gbuffer_targets, pack_draw_commands, pack_materials, pack_texture, raster_draws, to_device
    w, h = GBUFFER_W, GBUFFER_H
    rng = np.random.default_rng(2162)
    cb = np.zeros(152, np.float32)
    cb[:16] = np.eye(4, dtype=np.float32).reshape(-1)
    cb[64:68], cb[80:83], cb[104], cb[105], cb[106], cb[107] = (0.8, 0.7, 0.6, 1.0), (0.1, 0.2, 0.3), 0.25, 0.5, 1.0, 0.5
    for at in (112, 120, 128, 136):
        cb[at + 2], cb[at + 3], cb[at + 4] = 1.0, 1.0, 1.0
    constants = to_device(cb)
    pos = camera_space(triangles(rng, a.small, 0.125, 8.0, w, h))
    v = np.zeros((pos.shape[0], 16), np.float32)
    v[:, :3], v[:, 5] = pos, -1.0
    v[:, 6], v[:, 7] = pos[:, 0] / pos[:, 2] * (0.5 * w / 256.0), pos[:, 1] / pos[:, 2] * (0.5 * h / 256.0 * 2.5)
    v[:, 8], v[:, 11], v[:, 12:16] = 1.0, 1.0, 1.0
    vb, ib = to_device(v.reshape(-1)), to_device(np.arange(pos.shape[0], dtype=np.uint32))
    n, masked_slots = 8, (2, 5, 7)
    cuts = (np.linspace(0, pos.shape[0] // 3, n + 1).astype(int) * 3).tolist()
    cmds = to_device(pack_draw_commands([dict(vertices=vb, indices=ib, constants=constants, stride=64, start_index=cuts[k], index_count=cuts[k + 1] - cuts[k]) for k in range(n)]))
    tex = pack_texture([rng.integers(0, 256, (max(1, 1024 >> k), max(1, 1024 >> k), 4), dtype=np.uint8) for k in range(11)], True)
    table = lambda masked: pack_materials([{"key": 31 if masked and k in masked_slots else 15, "base_color": tex, "emissive": tex, "metallic_roughness": tex,  # noqa: E731
                                            "normal": tex} for k in range(n)])
    with_mask, without = table(True), table(False)

    def ranges(slots):
        return (to_device(np.array(list(slots) + [n], np.uint32)), cmds, to_device(np.ones(len(slots), np.uint32)))

    opaque, masked = ranges([k for k in range(n) if k not in masked_slots]), ranges(masked_slots)
    mask_draws = raster_draws(None, None, None, masked, 0)
    sets = []
    for _ in range(a.ring):
        ga, gb, hdr = (torch.empty((h, w, 4), dtype=torch.float16, device="cuda") for _ in range(3))
        gc, keys = (torch.zeros((h, w), dtype=torch.int32, device="cuda") for _ in range(2))
        sets.append((torch.zeros((h, w), dtype=torch.float32, device="cuda"), gbuffer_targets(ga, gb, gc, hdr, keys), torch.zeros((h, w), dtype=torch.int64, device="cuda")))
    mstats, won = torch.zeros(6, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    RASTER = lib.UR_GBUFFER_PART_RASTER
    hp.raster_reserve(a.reserve)

    def pre(i, sel):
        hp.depth_prepass(VIEW, PROJ, None if sel is not None else cmds, sets[i % a.ring][0], ranges=sel)

    def masked_call(i, parts, st=None, wn=None):
        pre(i, opaque)
        d, tg, k64 = sets[i % a.ring]
        hp.gbuffer_pass(VIEW, PROJ, None, d, tg, w, h, ranges=opaque, parts=parts, materials=with_mask, mask_draws=mask_draws, keys64=k64, mask_stats=st, won=wn)

    def opaque_call(i, parts):
        pre(i, None)
        d, tg, _ = sets[i % a.ring]
        hp.gbuffer_pass(VIEW, PROJ, cmds, d, tg, w, h, parts=parts, materials=without)

    masked_call(0, None, mstats, won)
    torch.cuda.synchronize()
    seen, texels_won = mstats.cpu().numpy().view(np.uint32).tolist(), int(won.cpu().numpy().view(np.uint32)[0])
    fns = {"DepthPrepass of the opaque draws": lambda i: pre(i, opaque),
           "DepthPrepass of the opaque draws + raster part with the mask": lambda i: masked_call(i, RASTER),
           "DepthPrepass of the opaque draws + whole ur_gbuffer_pass_masked": lambda i: masked_call(i, None),
           "DepthPrepass of all draws": lambda i: pre(i, None),
           "DepthPrepass of all draws + raster part, bit 4 cleared": lambda i: opaque_call(i, RASTER),
           "DepthPrepass of all draws + whole ur_gbuffer_pass_materials, bit 4 cleared": lambda i: opaque_call(i, None)}
    times = {k: [] for k in fns}
    for f in fns.values():
        f(0)
    torch.cuda.synchronize()
    for _ in range(a.batches):
        for k, f in fns.items():
            times[k].append(time_batch(torch, f, a.iters))
    return [{"shape": f"{w}x{h}, gbuffer masked, small, {k}", "median_us": float(np.median(t)), "min_us": float(np.min(t)), "max_us": float(np.max(t)), "stats_one_call": seen if "mask" in k else [],
             "batches": len(t), "calls_per_batch": a.iters, "maps": a.ring, "won": texels_won, "masked_commands": len(masked_slots), "commands": n} for k, t in times.items()]


def forward_leg(a, torch, hp):
    """The rows of --pass forward: at 3840 x 2160 over cold target sets, the small-triangle workload cut into 8 commands as the masked leg
    cuts it (--textured: pipeline key 15 on one 1024 x 1024 chain of random bytes; --masked: slots 2, 5 and 7 are the masked selection, key
    bit 4 set), rasterised once per set by the raster part of ur_forward_pass behind its DepthPrepass. Then, batch by batch in the same
    process over the same keys (and keys64): the forward resolve alone (ur_forward_pass_parts), the GBuffer resolve alone, ur_deferred_lighting
    alone over the G-buffer that resolve left, and the last two back to back: what the deferred path spends between the keys and the lit HDR.
    The tables are the shipped shapes with procedural content: a 2048 x 2048 shadow map, a 256-texel 9-mip cube, the 128 x 32 LUT."""
    from unclerenderer_amd import lib, synth
    from unclerenderer_amd.hotpath import forward_targets, gbuffer_targets, pack_draw_commands, pack_materials, pack_texture, pack_texture_bc, raster_draws, to_device
    w, h = GBUFFER_W, GBUFFER_H
    rng = np.random.default_rng(2163)
    cb = np.zeros(152, np.float32)
    cb[:16] = np.eye(4, dtype=np.float32).reshape(-1)
    cb[64:68], cb[80:83], cb[104], cb[105], cb[106], cb[107] = (0.8, 0.7, 0.6, 1.0), (0.1, 0.2, 0.3), 0.25, 0.5, 1.0, 0.5
    for at in (112, 120, 128, 136):
        cb[at + 2], cb[at + 3], cb[at + 4] = 1.0, 1.0, 1.0
    constants = to_device(cb)
    pos = camera_space(triangles(rng, a.small, 0.125, 8.0, w, h))
    v = np.zeros((pos.shape[0], 16), np.float32)
    v[:, :3], v[:, 5] = pos, -1.0
    v[:, 6], v[:, 7] = pos[:, 0] / pos[:, 2] * (0.5 * w / 256.0), pos[:, 1] / pos[:, 2] * (0.5 * h / 256.0 * 2.5)
    v[:, 8], v[:, 11], v[:, 12:16] = 1.0, 1.0, 1.0
    vb, ib = to_device(v.reshape(-1)), to_device(np.arange(pos.shape[0], dtype=np.uint32))
    n, masked_slots = 8, ((2, 5, 7) if a.masked else ())
    cuts = (np.linspace(0, pos.shape[0] // 3, n + 1).astype(int) * 3).tolist()
    cmds = to_device(pack_draw_commands([dict(vertices=vb, indices=ib, constants=constants, stride=64, start_index=cuts[k], index_count=cuts[k + 1] - cuts[k]) for k in range(n)]))
    materials = None
    if a.textured or a.masked:
        if a.bc:  # the one chain as random blocks
            data, fmt, _ = bc_chain_1024(rng, a.bc, True)
            tex = pack_texture_bc(data, 1024, 1024, 11, fmt)
        else:
            tex = pack_texture([rng.integers(0, 256, (max(1, 1024 >> k), max(1, 1024 >> k), 4), dtype=np.uint8) for k in range(11)], True)
        maps = {"base_color": tex, "emissive": tex, "metallic_roughness": tex, "normal": tex} if a.textured else {}
        materials = pack_materials([{"key": (15 if a.textured else 0) | (16 if k in masked_slots else 0), **maps} for k in range(n)])

    def ranges(slots):
        return (to_device(np.array(list(slots) + [n], np.uint32)), cmds, to_device(np.ones(len(slots), np.uint32)))

    opaque = ranges([k for k in range(n) if k not in masked_slots])
    mask_draws = raster_draws(None, None, None, ranges(masked_slots), 0) if a.masked else None
    scene = lib.SceneConstants()
    for name in ("World", "View", "ViewInverse"):
        getattr(scene, name)[:] = VIEW.tolist()
    scene.Projection[:] = PROJ.tolist()
    scene.LightDirection[:], scene.LightColor[:], scene.LightIntensity = (0.3, 0.8, -0.5), (1.0, 0.95, 0.85), 3.0
    scene.LightViewProjection[:] = [0.4, 0, 0, 0, 0, 0.4, 0, 0, 0, 0, 0.3, 0, 0, 0, 0.1, 1]
    scene.ShadowStrength, scene.ShadowBias, scene.EnvMapMipCount = 0.8, 0.002, 9.0
    scene.ShadowMapSize[:] = (2048.0, 2048.0)
    tables = hp.make_tables(to_device(synth.shadow_map_noise(2048, 1)), hp.stage_env_cube(synth.env_cube_procedural(256, 9), 256, 9), 256, 9,
                            to_device(synth.brdf_lut_procedural(128, 32)))
    sets = []
    for _ in range(a.ring):
        ga, gb, hdr, lit = (torch.zeros((h, w, 4), dtype=torch.float16, device="cuda") for _ in range(4))
        gc, keys = (torch.zeros((h, w), dtype=torch.int32, device="cuda") for _ in range(2))
        sets.append(dict(depth=torch.zeros((h, w), dtype=torch.float32, device="cuda"), gbuffer=gbuffer_targets(ga, gb, gc, hdr, keys), forward=forward_targets(lit, keys),
                         keys64=torch.zeros((h, w), dtype=torch.int64, device="cuda"), a=ga, b=gb, c=gc, hdr=hdr))
    RASTER, RESOLVE = lib.UR_GBUFFER_PART_RASTER, lib.UR_GBUFFER_PART_RESOLVE
    hp.raster_reserve(a.reserve)

    def forward(i, parts):
        s = sets[i % a.ring]
        mask = dict(mask_draws=mask_draws, keys64=s["keys64"]) if a.masked else {}
        hp.forward_pass(VIEW, PROJ, None, s["depth"], s["forward"], w, h, scene=scene, tables=tables, ranges=opaque, parts=parts, materials=materials, **mask)

    def resolve(i):
        s = sets[i % a.ring]
        mask = dict(mask_draws=mask_draws, keys64=s["keys64"]) if a.masked else {}
        hp.gbuffer_pass(VIEW, PROJ, None, s["depth"], s["gbuffer"], w, h, ranges=opaque, parts=RESOLVE, materials=materials, **mask)

    def lighting(i):
        s = sets[i % a.ring]
        hp.deferred_lighting(scene, s["a"], s["b"], s["c"], tables, s["hdr"], w, h)

    for i in range(a.ring):
        hp.depth_prepass(VIEW, PROJ, None, sets[i]["depth"], ranges=opaque)
        forward(i, RASTER)
    torch.cuda.synchronize()
    drawn = int((sets[0]["forward"]._keep[1] != 0).sum())
    fns = {"forward resolve": lambda i: forward(i, RESOLVE), "GBuffer resolve": resolve, "ur_deferred_lighting": lighting,
           "GBuffer resolve + ur_deferred_lighting": lambda i: (resolve(i), lighting(i))}
    times = {k: [] for k in fns}
    for f in fns.values():
        f(0)
    torch.cuda.synchronize()
    for _ in range(a.batches):
        for k, f in fns.items():
            times[k].append(time_batch(torch, f, a.iters))
    kind = f"{'textured' if a.textured else 'untextured'}{f' BC{a.bc}' if a.bc else ''}{', masked' if a.masked else ''}"
    return [{"shape": f"{w}x{h}, forward, small, {kind}, {k}", "median_us": float(np.median(t)), "min_us": float(np.min(t)), "max_us": float(np.max(t)), "stats_one_call": [], "batches": len(t),
             "calls_per_batch": a.iters, "maps": a.ring, "texels_drawn": drawn} for k, t in times.items()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10, help="calls per timed batch")
    ap.add_argument("--ring", type=int, default=4, help="maps cycled through so that every call meets a cold map")
    ap.add_argument("--small", type=int, default=1_000_000)
    ap.add_argument("--reserve", type=int, default=1 << 19)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--pass", dest="which", choices=("shadow", "depth", "both", "gbuffer", "forward"), default="shadow")
    ap.add_argument("--textured", action="store_true", help="with --pass gbuffer: the textured resolve beside the untextured one; with --pass forward: key 15")
    ap.add_argument("--masked", action="store_true", help="with --pass gbuffer: the alpha-masked raster beside the all-opaque one; with --pass forward: a masked selection")
    ap.add_argument("--bc", type=int, choices=(1, 3, 5), default=0, help="with --textured: the maps as random BC1 / BC3 / BC5 blocks instead of RGBA8 texels")
    ap.add_argument("--no-probe-count", action="store_true", help="with --textured: skip the host-side mean probe count")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    if a.bc and not (a.textured and a.which in ("gbuffer", "forward")):
        ap.error("--bc goes with --pass gbuffer --textured or --pass forward --textured")
    if a.quick:
        a.batches, a.iters, a.ring = 1, 2, 2
    import torch
    from unclerenderer_amd.hotpath import HotPath, pack_draw_commands, to_device
    assert torch.cuda.is_available(), "bench_shadow needs a GPU"
    hp = HotPath(0)
    rng = np.random.default_rng(2048)
    world = to_device(np.eye(4, dtype=np.float32).reshape(-1))
    lvp = np.eye(4, dtype=np.float32).reshape(-1)

    def mesh(pos):
        v = np.zeros((pos.shape[0], 16), np.float32)
        v[:, :3] = pos
        vb, ib = to_device(v.reshape(-1)), to_device(np.arange(pos.shape[0], dtype=np.uint32))
        return dict(vertices=vb, indices=ib, constants=world, stride=64)

    view, proj = VIEW, PROJ

    small_pos, large_pos = triangles(rng, a.small, 0.125, 8.0), triangles(rng, 256, SIZE, 2 * SIZE)
    legs = []
    if a.which in ("shadow", "both"):
        small, large = mesh(small_pos), mesh(large_pos)
        legs.append(("", 4, {"small": [small], "large": [large], "mix": [small, large]},
                     lambda c, m, st: hp.shadow_map(lvp, c, m, stats=st, command_count=None if c is not None else 0)))
    if a.which in ("depth", "both"):
        small, large = mesh(camera_space(small_pos)), mesh(camera_space(large_pos))
        legs.append(("depth prepass, ", 6, {"small": [small], "large": [large], "mix": [small, large]},
                     lambda c, m, st: hp.depth_prepass(view, proj, c, m, stats=st, command_count=None if c is not None else 0)))
    maps = [torch.empty((SIZE, SIZE), dtype=torch.float32, device="cuda") for _ in range(a.ring)]
    rows = []
    for label, nstats, loads, call in legs:
        cmds = {k: to_device(pack_draw_commands(v)) for k, v in loads.items()}
        stats = torch.zeros(nstats, dtype=torch.int32, device="cuda")
        for reserve in (a.reserve, 0):
            hp.raster_reserve(reserve)
            shapes = {"clear alone": None, **cmds}
            fns = {k: (lambda i, c=c: call(c, maps[i % a.ring], stats if c is not None else None)) for k, c in shapes.items()}
            seen = {}
            for k, f in fns.items():
                stats.zero_()
                f(0)
                torch.cuda.synchronize()
                seen[k] = stats.cpu().numpy().view(np.uint32).tolist()
            times = {k: [] for k in fns}
            for _ in range(a.batches):
                for k, f in fns.items():
                    times[k].append(time_batch(torch, f, a.iters))
            for k, t in times.items():
                rows.append({"shape": f"{SIZE}x{SIZE}, {label}{k}, reserve {reserve}", "median_us": float(np.median(t)), "min_us": float(np.min(t)),
                             "stats_one_call": seen[k], "batches": len(t), "calls_per_batch": a.iters, "maps": a.ring})
    if a.which == "gbuffer":
        rows += gbuffer_masked_leg(a, torch, hp) if a.masked else (gbuffer_textured_leg(a, torch, hp) if a.textured else gbuffer_leg(a, torch, hp))
    if a.which == "forward":
        rows += forward_leg(a, torch, hp)
    hp.raster_reserve(0)
    hp.close()
    for r in rows:
        print(f"{r['shape']:{96 if a.which in ('gbuffer', 'forward') else 64}s} median {r['median_us']:10.2f} us  min {r['min_us']:10.2f} us  stats {r['stats_one_call']}")
    if a.json:
        with open(a.json, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    print(json.dumps({"tool": "bench_shadow", "quick": a.quick, "results": rows}))


if __name__ == "__main__":
    main()
