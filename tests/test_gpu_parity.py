"""GPU parity tests: the HIP path (through the C-ABI) against the CPU oracle on the same seeded inputs.

Bars (BASELINE.json north_star): bit-exact for the HZB, the InstanceCount words, the visible list and its count;
max(1e-3, 1 fp16 ulp) per channel for the RGBA16F HDR target. The oracle is unpinned by the reference (no tests or
golden vectors exist there); it is pinned by tests/test_oracle_*.py and tests/golden/.
"""
import ctypes as C

import numpy as np
import pytest

from tests.util import hdr_mismatch

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    return torch


# ---------------------------------------------------------------------------------------------------------------------
# BuildHZB
# ---------------------------------------------------------------------------------------------------------------------
HZB_SIZES = [(1, 1), (2, 2), (3, 5), (17, 9), (64, 64), (129, 67), (512, 512), (1920, 1080), (1000, 3), (5, 300), (2, 33), (4096, 16),
             (6001, 3999), (7680, 4320),  # mip 4 is too large for the tail's LDS, mip 5 fits: five levels, then the tail reads mip 4 from memory (two launches)
             (16384, 4200)]  # mip 5 (256 x 65) is too large as well: four levels, four more from mip 3, then the tail (three launches)


@pytest.mark.parametrize("w,h", HZB_SIZES)
def test_build_hzb_bit_exact(hotpath, oracle, w, h):
    from unclerenderer_amd.hotpath import HzbLayout, to_device
    torch = _torch()
    rng = np.random.default_rng(1000 + w * 7 + h)
    depth = rng.random((h, w), dtype=np.float32)
    depth[rng.random((h, w)) < 0.1] = 0.0  # cleared pixels
    lay = HzbLayout(w, h)
    # sizing == CreateHZBResources (oracle restates it independently, packed)
    packed, _ = oracle.hzb_layout(w, h)
    assert [(m[1], m[2]) for m in packed] == [(m[1], m[2]) for m in lay.as_list()]
    hzb = torch.full((lay.total,), float("nan"), dtype=torch.float32, device="cuda")
    hotpath.build_hzb(to_device(depth), hzb, lay)
    torch.cuda.synchronize()
    got = hzb.cpu().numpy()
    ref = oracle.build_hzb(depth, lay.as_list(), lay.total)
    for (off, mw, mh) in lay.as_list():
        a = got[off:off + mw * mh].view(np.uint32)
        b = ref[off:off + mw * mh].view(np.uint32)
        assert np.array_equal(a, b), f"mip {mw}x{mh} differs at {np.flatnonzero(a != b)[:8]}"
    # nothing outside the mips is written
    mask = np.ones(lay.total, bool)
    for (off, mw, mh) in lay.as_list():
        mask[off:off + mw * mh] = False
    assert np.isnan(got[mask]).all()


def test_build_hzb_rejects_bad_chain(hotpath):
    from unclerenderer_amd import lib
    from unclerenderer_amd.hotpath import HzbLayout
    torch = _torch()
    lay = HzbLayout(64, 64)
    lay.mips[1].width += 1
    d = torch.zeros(64 * 64, device="cuda")
    hz = torch.zeros(lay.total + 64, device="cuda")
    with pytest.raises(lib.UrError) as e:
        hotpath.build_hzb(d, hz, lay)
    assert e.value.code == lib.UR_EINVAL


# ---------------------------------------------------------------------------------------------------------------------
# CullIndirectArgs + compaction
# ---------------------------------------------------------------------------------------------------------------------
def _cull_case(hotpath, oracle, n, hzb_on, seed, w=480, h=270, debug=True, index_base=0, box=120.0):
    from unclerenderer_amd import hostmath, synth
    from unclerenderer_amd.hotpath import HzbLayout, to_device
    torch = _torch()
    fc = hostmath.build_frame_constants("sponza", w, h)
    g = synth.gbuffer_scene(fc.view, fc.proj, fc.camera_position, w, h, seed)
    lay = HzbLayout(w, h)
    hzb_ref = oracle.build_hzb(g.depth, lay.as_list(), lay.total)
    hzb_ref = np.nan_to_num(hzb_ref, nan=0.0)
    bounds = synth.instances_random(n, seed, center=fc.camera_position, box=box)
    consts = hostmath.pack_culling_constants(fc.view, fc.proj, n, hzb_on, lay.count, lay.width, lay.height, debug)
    args0 = synth.indirect_args_initial(n)
    ref_args, ref_stats, ref_vis, ref_cnt = oracle.cull_indirect_args(consts, bounds, hzb_ref, lay.as_list(), args0, index_base)

    d_args = to_device(args0)
    d_stats = torch.zeros(2, dtype=torch.int32, device="cuda")
    d_vis = torch.full((max(n, 1),), -1, dtype=torch.int32, device="cuda")
    d_cnt = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    hotpath.cull_indirect_args(consts, to_device(bounds), to_device(hzb_ref), lay, d_args, d_stats, d_vis, d_cnt, index_base)
    torch.cuda.synchronize()
    got_args = d_args.cpu().numpy().view(np.uint32)
    assert np.array_equal(got_args, ref_args), "indirect args differ (InstanceCount words or bytes outside offset 44)"
    cnt = int(d_cnt.cpu().numpy().view(np.uint32)[0])
    assert cnt == ref_cnt
    got_vis = d_vis.cpu().numpy().view(np.uint32)[:cnt]
    assert np.array_equal(got_vis, ref_vis)
    assert np.array_equal(d_stats.cpu().numpy().view(np.uint32), ref_stats)
    # definition of the derived list
    words = ref_args[:, 11]
    assert np.array_equal(ref_vis, np.flatnonzero(words == 1).astype(np.uint32) + index_base)
    return ref_cnt, ref_stats


@pytest.mark.parametrize("n", [25, 257, 20_000])
def test_cull_store_flavours_leave_the_same_bytes(hotpath, oracle, n):
    """UR_OPT_CULL_STORE 0..3 (plain, nontemporal, write-through, write-through of changed words only - the default): whatever the
    InstanceCount words hold when the launch starts (the reference's 1, last frame's result, zeros, garbage), the command buffer ends
    up byte-equal to the oracle's, dword 11 and everything around it."""
    from unclerenderer_amd import hostmath, lib, synth
    from unclerenderer_amd.hotpath import HzbLayout, to_device
    torch = _torch()
    w, h = 480, 270
    fc = hostmath.build_frame_constants("sponza", w, h)
    g = synth.gbuffer_scene(fc.view, fc.proj, fc.camera_position, w, h, 11)
    lay = HzbLayout(w, h)
    hzb_ref = np.nan_to_num(oracle.build_hzb(g.depth, lay.as_list(), lay.total), nan=0.0)
    bounds = synth.instances_random(n, 11 + n, center=fc.camera_position, box=120.0)
    consts = hostmath.pack_culling_constants(fc.view, fc.proj, n, True, lay.count, lay.width, lay.height, False)
    args0 = synth.indirect_args_initial(n)
    ref_args, _, ref_vis, ref_cnt = oracle.cull_indirect_args(consts, bounds, hzb_ref, lay.as_list(), args0, 0)
    assert hotpath.get_option(lib.UR_OPT_CULL_STORE) == 3
    d_bounds, d_hzb = to_device(bounds), to_device(hzb_ref)
    rng = np.random.default_rng(5)
    starts = {"ones": args0, "result": ref_args}
    for name, fill in (("zeros", 0), ("garbage", None)):
        a = args0.copy()
        a[:, 11] = fill if fill is not None else rng.integers(2, 2**32, n, dtype=np.uint64).astype(np.uint32)
        starts[name] = a
    try:
        for flavour in (0, 1, 2, 3):
            hotpath.set_option(lib.UR_OPT_CULL_STORE, flavour)
            for name, start in starts.items():
                d_args = to_device(np.ascontiguousarray(start))
                d_vis = torch.full((n,), -1, dtype=torch.int32, device="cuda")
                d_cnt = torch.full((1,), -1, dtype=torch.int32, device="cuda")
                hotpath.cull_indirect_args(consts, d_bounds, d_hzb, lay, d_args, None, d_vis, d_cnt, 0)
                torch.cuda.synchronize()
                got = d_args.cpu().numpy().view(np.uint32).reshape(n, 16)
                assert np.array_equal(got, ref_args), f"flavour {flavour}, start {name}"
                assert int(d_cnt.cpu().numpy().view(np.uint32)[0]) == ref_cnt
                assert np.array_equal(d_vis.cpu().numpy().view(np.uint32)[:ref_cnt], ref_vis)
    finally:
        hotpath.set_option(lib.UR_OPT_CULL_STORE, 3)


@pytest.mark.parametrize("with_list", [True, False])
def test_cull_store_from_the_contexts_record(hotpath, oracle, with_list):
    """UR_OPT_CULL_STORE = 4: the words' present values are taken from the context's one-bit-per-instance record of its previous launch on
    the same command buffer. A sequence that changes camera, buffer, count and (with the option set anew, as the contract asks) lets somebody
    else overwrite the words: after every launch the command buffer is byte-equal to the oracle's."""
    from unclerenderer_amd import hostmath, lib, synth
    from unclerenderer_amd.hotpath import HzbLayout, to_device
    torch = _torch()
    w, h, n = 480, 270, 5000
    lay = HzbLayout(w, h)
    cams = []
    for k, preset in enumerate(("sponza", "pica_pica")):
        fc = hostmath.build_frame_constants(preset, w, h)
        g = synth.gbuffer_scene(fc.view, fc.proj, fc.camera_position, w, h, 21 + k)
        hzb = np.nan_to_num(oracle.build_hzb(g.depth, lay.as_list(), lay.total), nan=0.0)
        cams.append((fc, hzb, to_device(hzb)))
    bounds = synth.instances_random(n, 77, center=cams[0][0].camera_position, box=120.0)
    d_bounds = to_device(bounds)
    args0 = synth.indirect_args_initial(n)
    rng = np.random.default_rng(9)
    garbage = args0.copy()
    garbage[:, 11] = rng.integers(0, 3, n).astype(np.uint32)
    bufs = {"x": to_device(args0), "y": to_device(garbage)}
    hotpath.set_option(lib.UR_OPT_CULL_STORE, 4)
    try:
        def launch(buf, cam, count):
            fc, hzb_ref, d_hzb = cams[cam]
            consts = hostmath.pack_culling_constants(fc.view, fc.proj, count, True, lay.count, lay.width, lay.height, False)
            d_vis = torch.full((n,), -1, dtype=torch.int32, device="cuda") if with_list else None
            d_cnt = torch.full((1,), -1, dtype=torch.int32, device="cuda") if with_list else None
            before = bufs[buf].cpu().numpy().view(np.uint32).reshape(n, 16).copy()
            hotpath.cull_indirect_args(consts, d_bounds, d_hzb, lay, bufs[buf], None, d_vis, d_cnt, 0)
            torch.cuda.synchronize()
            ref_args, _, ref_vis, ref_cnt = oracle.cull_indirect_args(consts, bounds[:count], hzb_ref, lay.as_list(), before[:count].copy(), 0)
            got = bufs[buf].cpu().numpy().view(np.uint32).reshape(n, 16)
            assert np.array_equal(got[:count], ref_args), f"buffer {buf}, camera {cam}, count {count}"
            assert np.array_equal(got[count:], before[count:]), "commands behind the count were touched"
            if with_list:
                assert int(d_cnt.cpu().numpy().view(np.uint32)[0]) == ref_cnt
                assert np.array_equal(d_vis.cpu().numpy().view(np.uint32)[:ref_cnt], ref_vis)
            return ref_args[:, 11].copy()

        a = launch("x", 0, n)      # no record yet: the words are read
        b = launch("x", 1, n)      # another camera, from the record
        assert (a != b).any(), "the two cameras must disagree on some instance for the record to matter"
        launch("x", 0, n)          # and back
        launch("y", 0, n)          # another buffer, arbitrary words in it: no record for it
        launch("y", 1, n)
        launch("x", 1, n)          # back on x: the record is y's, the words are read
        launch("x", 0, n - 300)    # a shorter count: no record
        launch("x", 1, n - 300)
        # somebody else rewrites the words; the caller says so by setting the option anew
        bufs["x"].copy_(to_device(garbage))
        hotpath.set_option(lib.UR_OPT_CULL_STORE, 4)
        launch("x", 1, n - 300)
        launch("x", 0, n - 300)
    finally:
        hotpath.set_option(lib.UR_OPT_CULL_STORE, 3)


@pytest.mark.parametrize("n", [1, 25, 63, 64, 65, 170, 256, 257, 1023, 4097, 100_000])
@pytest.mark.parametrize("hzb_on", [False, True])
def test_cull_bit_exact(hotpath, oracle, n, hzb_on):
    cnt, stats = _cull_case(hotpath, oracle, n, hzb_on, seed=7 + n)
    if n >= 1023:
        assert 0 < cnt < n, "the synthetic case must exercise both outcomes"
        if hzb_on:
            assert stats[1] > 0, "no instance was occlusion-culled: HZB path not exercised"


def test_cull_index_base_and_no_list(hotpath, oracle):
    _cull_case(hotpath, oracle, 5000, True, seed=99, index_base=123_456)
    # visible list is optional: words only
    from unclerenderer_amd import hostmath, synth
    from unclerenderer_amd.hotpath import to_device
    fc = hostmath.build_frame_constants("sponza", 64, 36)
    n = 700
    bounds = synth.instances_random(n, 5, center=fc.camera_position, box=60.0)
    consts = hostmath.pack_culling_constants(fc.view, fc.proj, n, False, 0, 0, 0, False)
    args0 = synth.indirect_args_initial(n)
    ref_args, *_ = oracle.cull_indirect_args(consts, bounds, None, [], args0)
    d_args = to_device(args0)
    hotpath.cull_indirect_args(consts, to_device(bounds), None, None, d_args)
    assert np.array_equal(d_args.cpu().numpy().view(np.uint32), ref_args)


def test_cull_empty(hotpath):
    from unclerenderer_amd import hostmath
    torch = _torch()
    fc = hostmath.build_frame_constants("sponza", 64, 36)
    consts = hostmath.pack_culling_constants(fc.view, fc.proj, 0, False, 0, 0, 0, False)
    d_cnt = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    d_vis = torch.zeros(1, dtype=torch.int32, device="cuda")
    hotpath.cull_indirect_args(consts, None, None, None, None, None, d_vis, d_cnt)
    assert int(d_cnt.cpu()[0]) == 0


def test_cull_sponza_25(hotpath, oracle):
    """BASELINE config 3's actual cull: 25 commands sharing one AABB."""
    from unclerenderer_amd import hostmath, synth
    from unclerenderer_amd.hotpath import to_device
    torch = _torch()
    p = hostmath.SCENES["sponza"]
    fc = hostmath.build_frame_constants(p, 3840, 2160)
    bounds = synth.instances_replicated(*p.model_aabb, p.instance_count)
    consts = hostmath.pack_culling_constants(fc.view, fc.proj, 25, False, 0, 0, 0, True)
    args0 = synth.indirect_args_initial(25)
    ref_args, ref_stats, ref_vis, ref_cnt = oracle.cull_indirect_args(consts, bounds, None, [], args0)
    assert ref_cnt == 25  # the camera is inside the model's box
    d_args = to_device(args0)
    d_vis = torch.zeros(25, dtype=torch.int32, device="cuda")
    d_cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    hotpath.cull_indirect_args(consts, to_device(bounds), None, None, d_args, None, d_vis, d_cnt)
    assert np.array_equal(d_args.cpu().numpy().view(np.uint32), ref_args)
    assert np.array_equal(d_vis.cpu().numpy().view(np.uint32), ref_vis)


# ---------------------------------------------------------------------------------------------------------------------
# DeferredLighting / SkyAtmosphere
# ---------------------------------------------------------------------------------------------------------------------
def _lighting_inputs(scene_name, w, h, seed, mode, shadow_size=256, shadow_strength=1.0):
    from unclerenderer_amd import hostmath, synth
    fc = hostmath.build_frame_constants(scene_name, w, h, shadow_size=shadow_size, shadow_strength=shadow_strength)
    if mode == "iid":
        g = synth.gbuffer_iid(w, h, seed)
    else:
        g = synth.gbuffer_scene(fc.view, fc.proj, fc.camera_position, w, h, seed)
    shadow = synth.shadow_map_noise(shadow_size, seed)
    env = synth.env_cube_procedural(32, 6)
    lut = synth.brdf_lut_procedural(128, 32)
    fc.scene.EnvMapMipCount = 6.0
    return fc, g, shadow, env, lut


def _device_tables(hotpath, shadow, env, lut, base=32, mips=6):
    from unclerenderer_amd.hotpath import to_device
    d_env = hotpath.stage_env_cube(env, base, mips)
    return hotpath.make_tables(to_device(shadow) if shadow is not None else None, d_env, base, mips, to_device(lut))


@pytest.mark.parametrize("mode", ["iid", "scene"])
@pytest.mark.parametrize("scene_name", ["sponza", "duck"])
def test_lighting_and_sky_parity(hotpath, oracle, mode, scene_name):
    from unclerenderer_amd.hotpath import to_device
    torch = _torch()
    w, h = 256, 144
    fc, g, shadow, env, lut = _lighting_inputs(scene_name, w, h, seed=11, mode=mode)
    tables = _device_tables(hotpath, shadow, env, lut)
    dA, dB, dC, dD = to_device(g.A), to_device(g.B), to_device(g.C), to_device(g.depth)

    # --- lighting only (every pixel, NaN on cleared pixels like the reference)
    ref_l, fragile = oracle.deferred_lighting(fc.scene, g.A, g.B, g.C, shadow, env, 32, 6, lut, g.hdr, w, h, want_fragile=True)
    d_hdr = to_device(g.hdr)
    hotpath.deferred_lighting(fc.scene, dA, dB, dC, tables, d_hdr, w, h)
    torch.cuda.synchronize()
    got_l = d_hdr.cpu().numpy().view(np.uint16)
    nbad, worst, _ = hdr_mismatch(got_l, ref_l, exclude=fragile)
    assert nbad == 0, f"lighting: {nbad} channel values beyond tolerance (worst excess {worst})"
    assert fragile.mean() < 5e-3
    bg = g.depth == 0
    if bg.any():
        assert np.isnan(got_l.view(np.float16)[bg][:, :3].astype(np.float32)).all(), "cleared pixels must shade to NaN"

    # --- sky over the lit buffer
    ref_s = oracle.sky_atmosphere(fc.sky, g.depth, ref_l, w, h)
    hotpath.sky_atmosphere(fc.sky, dD, d_hdr, w, h)
    torch.cuda.synchronize()
    got_s = d_hdr.cpu().numpy().view(np.uint16)
    nbad, worst, _ = hdr_mismatch(got_s, ref_s, exclude=fragile)
    assert nbad == 0, f"sky: {nbad} beyond tolerance (worst {worst})"
    assert not np.isnan(got_s.view(np.float16).astype(np.float32)[~fragile.astype(bool)]).any()

    # --- fused == the two passes
    d_hdr2 = to_device(g.hdr)
    hotpath.deferred_lighting_sky(fc.scene, fc.sky, dA, dB, dC, dD, tables, d_hdr2, w, h)
    torch.cuda.synchronize()
    got_f = d_hdr2.cpu().numpy().view(np.uint16)
    nbad, worst, _ = hdr_mismatch(got_f, ref_s, exclude=fragile)
    assert nbad == 0, f"fused: {nbad} beyond tolerance (worst {worst})"
    assert np.array_equal(got_f, got_s), "fused kernel must equal lighting followed by sky bit for bit"


def test_lighting_without_shadows(hotpath, oracle):
    from unclerenderer_amd.hotpath import to_device
    torch = _torch()
    w, h = 128, 64
    fc, g, shadow, env, lut = _lighting_inputs("sponza", w, h, seed=3, mode="iid", shadow_strength=0.0)
    tables = _device_tables(hotpath, None, env, lut)
    ref = oracle.deferred_lighting(fc.scene, g.A, g.B, g.C, None, env, 32, 6, lut, g.hdr, w, h)
    d_hdr = to_device(g.hdr)
    hotpath.deferred_lighting(fc.scene, to_device(g.A), to_device(g.B), to_device(g.C), tables, d_hdr, w, h)
    torch.cuda.synchronize()
    nbad, worst, _ = hdr_mismatch(d_hdr.cpu().numpy().view(np.uint16), ref)
    assert nbad == 0, (nbad, worst)


@pytest.mark.parametrize("w,h", [(16, 1), (16, 5), (32, 3), (48, 7), (64, 4), (272, 33), (24, 9), (130, 3), (1, 1)])
@pytest.mark.parametrize("mode", ["scene", "iid"])
def test_lighting_tile_geometry(hotpath, oracle, w, h, mode):
    """The streaming lighting kernel walks 16x4-pixel tiles (partial bottom tiles hang over the band); widths that are
    not a multiple of 16 take the per-tile kernel. Every shape agrees with the oracle, fused and lighting-only."""
    from unclerenderer_amd.hotpath import to_device
    torch = _torch()
    fc, g, shadow, env, lut = _lighting_inputs("sponza", w, h, seed=100 + w + h, mode=mode)
    tables = _device_tables(hotpath, shadow, env, lut)
    ref_l, fragile = oracle.deferred_lighting(fc.scene, g.A, g.B, g.C, shadow, env, 32, 6, lut, g.hdr, w, h, want_fragile=True)
    ref_s = oracle.sky_atmosphere(fc.sky, g.depth, ref_l, w, h)
    dA, dB, dC, dD = to_device(g.A), to_device(g.B), to_device(g.C), to_device(g.depth)
    d1, d2 = to_device(g.hdr), to_device(g.hdr)
    hotpath.deferred_lighting(fc.scene, dA, dB, dC, tables, d1, w, h)
    hotpath.deferred_lighting_sky(fc.scene, fc.sky, dA, dB, dC, dD, tables, d2, w, h)
    torch.cuda.synchronize()
    nbad, worst, _ = hdr_mismatch(d1.cpu().numpy().view(np.uint16), ref_l, exclude=fragile)
    assert nbad == 0, f"lighting {w}x{h}: {nbad} beyond tolerance (worst {worst})"
    nbad, worst, _ = hdr_mismatch(d2.cpu().numpy().view(np.uint16), ref_s, exclude=fragile)
    assert nbad == 0, f"fused {w}x{h}: {nbad} beyond tolerance (worst {worst})"


def test_lighting_band_offsets(hotpath, oracle):
    """A band that starts in the middle of the frame and is not a multiple of the tile height (a 1-of-8 shard of 1080p)."""
    from unclerenderer_amd.hotpath import to_device
    torch = _torch()
    w, h, r0, rows = 320, 270, 135, 34
    fc, g, shadow, env, lut = _lighting_inputs("sponza", w, h, seed=9, mode="scene")
    tables = _device_tables(hotpath, shadow, env, lut)
    sl = slice(r0, r0 + rows)
    ref_l, fragile = oracle.deferred_lighting(fc.scene, g.A[sl], g.B[sl], g.C[sl], shadow, env, 32, 6, lut, g.hdr[sl], w, h, r0, rows, want_fragile=True)
    ref = oracle.sky_atmosphere(fc.sky, g.depth[sl], ref_l, w, h, r0, rows)
    out = to_device(g.hdr[sl])
    hotpath.deferred_lighting_sky(fc.scene, fc.sky, to_device(g.A[sl]), to_device(g.B[sl]), to_device(g.C[sl]), to_device(g.depth[sl]), tables, out, w, h, r0, rows)
    torch.cuda.synchronize()
    nbad, worst, _ = hdr_mismatch(out.cpu().numpy().view(np.uint16), ref, exclude=fragile)
    assert nbad == 0, (nbad, worst)


def test_lighting_shadow_border_and_outside(hotpath, oracle):
    """A small shadow map whose frustum does not cover the view: PCF footprints on the border (opaque white) and pixels
    outside the map (shadow = 1) take the slow path of both kernels."""
    from unclerenderer_amd.hotpath import to_device
    torch = _torch()
    w, h = 192, 108
    fc, g, shadow, env, lut = _lighting_inputs("duck", w, h, seed=17, mode="scene", shadow_size=8)
    tables = _device_tables(hotpath, shadow, env, lut)
    ref_l, fragile = oracle.deferred_lighting(fc.scene, g.A, g.B, g.C, shadow, env, 32, 6, lut, g.hdr, w, h, want_fragile=True)
    d = to_device(g.hdr)
    hotpath.deferred_lighting(fc.scene, to_device(g.A), to_device(g.B), to_device(g.C), tables, d, w, h)
    torch.cuda.synchronize()
    nbad, worst, _ = hdr_mismatch(d.cpu().numpy().view(np.uint16), ref_l, exclude=fragile)
    assert nbad == 0, (nbad, worst)
    # an 8x8 map stretched over the whole view: a texel edge (where the PCF compare may flip within 1e-5) crosses most of the
    # 192x108 pixels' footprints, so the flagged share is large HERE; the full-size configurations flag < 0.5 % (test_gpu_configs)
    assert fragile.mean() < 0.05
    assert (~fragile.astype(bool)).sum() > 0.9 * w * h


def test_streaming_and_per_tile_kernels_agree(hotpath, oracle):
    """The two lighting kernels are independent implementations of the same pass (the per-tile one serves sky-only launches
    and the configurations the streaming kernel declines): on the same inputs EACH is within the HDR tolerance of the
    oracle on every pixel that is not shadow-compare fragile, hence they are within twice that of each other.
    The per-tile kernel is selected on the same context with ur_set_option(UR_OPT_LIGHTING_STREAM, 0)."""
    from tests.util import fp16_ulp, half_to_f32
    from unclerenderer_amd import lib
    from unclerenderer_amd.hotpath import to_device
    torch = _torch()
    w, h = 320, 180
    fc, g, shadow, env, lut = _lighting_inputs("sponza", w, h, seed=33, mode="scene")
    tables = _device_tables(hotpath, shadow, env, lut)
    bits = {}
    try:
        for name, stream in (("streaming", 1), ("per-tile", 0)):
            hotpath.set_option(lib.UR_OPT_LIGHTING_STREAM, stream)
            assert hotpath.get_option(lib.UR_OPT_LIGHTING_STREAM) == stream
            out = to_device(g.hdr)
            hotpath.deferred_lighting_sky(fc.scene, fc.sky, to_device(g.A), to_device(g.B), to_device(g.C), to_device(g.depth), tables, out, w, h)
            torch.cuda.synchronize()
            bits[name] = out.cpu().numpy().view(np.uint16)
    finally:
        hotpath.set_option(lib.UR_OPT_LIGHTING_STREAM, 1)
    stream_bits, tile_bits = bits["streaming"], bits["per-tile"]
    lit, frag = oracle.deferred_lighting(fc.scene, g.A, g.B, g.C, shadow, env, 32, 6, lut, g.hdr, w, h, want_fragile=True)
    ref = oracle.sky_atmosphere(fc.sky, g.depth, lit, w, h)
    for name, bits in (("streaming", stream_bits), ("per-tile", tile_bits)):
        nbad, worst, _ = hdr_mismatch(bits, ref, exclude=frag)
        assert nbad == 0, f"{name} kernel: {nbad} channel values beyond tolerance of the oracle (worst excess {worst})"
    a, b, r32 = half_to_f32(stream_bits), half_to_f32(tile_bits), half_to_f32(ref)
    keep = ~frag.astype(bool)
    assert (np.abs(a - b)[keep] <= 2.0 * np.maximum(np.float32(1e-3), fp16_ulp(r32))[keep]).all()
    assert frag.mean() < 5e-3


def test_row_bands_equal_whole_frame(hotpath):
    """Screen-tile sharding: shading 4 bands separately gives the whole-frame result bit for bit."""
    from unclerenderer_amd.hotpath import to_device
    torch = _torch()
    w, h = 320, 180
    fc, g, shadow, env, lut = _lighting_inputs("sponza", w, h, seed=21, mode="scene")
    tables = _device_tables(hotpath, shadow, env, lut)
    dA, dB, dC, dD = to_device(g.A), to_device(g.B), to_device(g.C), to_device(g.depth)
    whole = to_device(g.hdr)
    hotpath.deferred_lighting_sky(fc.scene, fc.sky, dA, dB, dC, dD, tables, whole, w, h)
    parts = to_device(g.hdr)
    for r in range(4):
        r0, rows = r * 45, 45
        sl = slice(r0, r0 + rows)
        hotpath.deferred_lighting_sky(fc.scene, fc.sky, dA[sl], dB[sl], dC[sl], dD[sl], tables, parts[sl], w, h, r0, rows)
    torch.cuda.synchronize()
    assert torch.equal(whole, parts)


def test_stage_env_cube_matches_folding_rule(hotpath, oracle):
    from unclerenderer_amd import synth
    env = synth.env_cube_procedural(16, 5)
    env[:, 0] = (np.arange(env.shape[0]) & 0x3FF).astype(np.uint16)  # make every texel distinguishable
    got = hotpath.stage_env_cube(env, 16, 5).cpu().numpy().view(np.uint16).reshape(-1, 4)
    ref = oracle.stage_env_cube(env, 16, 5).reshape(-1, 4)
    nb = ref.shape[0]
    assert np.array_equal(got[:nb], ref)  # the bordered faces
    # behind them the same faces as RGB row pairs: entry (f, j, i) = {R G B of texel (i, j), R G B of texel (i, j + 1)}, 12 bytes
    rgb = got[nb:].reshape(-1)  # uint16 stream
    off, boff = 0, 0
    for m in range(5):
        E = max(1, 16 >> m) + 2
        faces = ref[boff:boff + 6 * E * E].reshape(6, E, E, 4)[..., :3]
        pairs = np.stack([faces[:, :-1], faces[:, 1:]], axis=3)  # (6, E-1, E, 2, 3)
        n = 6 * E * (E - 1) * 6
        assert np.array_equal(rgb[off:off + n], pairs.reshape(-1)), m
        off += n; boff += 6 * E * E
    assert off == rgb.size


@pytest.mark.parametrize("case", ["sheared_view", "scaled_view", "camera_elsewhere", "shadow_2x2", "shadow_1x1", "shadow_2x5"])
def test_lighting_inputs_outside_the_fast_paths(hotpath, oracle, case):
    """What the reference never produces but its shader would shade all the same (DeferredLighting.hlsl:55,76-84): a
    ViewInverse that is not rigid, a CameraPosition that is not its origin, a shadow map too small for a 3x3 block. They take
    the per-tile kernel with the world-space vectors formed literally / every tap through the bordered PCF, and agree with the
    oracle like every other input (rounds 1-2 returned UR_EUNSUPPORTED)."""
    from unclerenderer_amd import synth
    from unclerenderer_amd.hotpath import to_device
    torch = _torch()
    w, h = 96, 40
    ss = {"shadow_2x2": (2, 2), "shadow_1x1": (1, 1), "shadow_2x5": (2, 5)}.get(case)
    fc, g, shadow, env, lut = _lighting_inputs("sponza", w, h, seed=21, mode="scene")
    if case == "sheared_view":
        fc.scene.ViewInverse[1] += 0.35   # row 0 no longer orthogonal to row 1
        fc.scene.ViewInverse[6] -= 0.2
    elif case == "scaled_view":
        for k in (0, 1, 2):
            fc.scene.ViewInverse[k] *= 1.7  # row 0 of the 3x3 scaled
    elif case == "camera_elsewhere":
        fc.scene.CameraPosition[0] += 3.0
        fc.scene.CameraPosition[1] -= 1.5
    else:
        sw, sh_ = ss
        shadow = (0.2 + 0.7 * np.random.default_rng(5).random((sh_, sw))).astype(np.float32)
        fc.scene.ShadowMapSize[0], fc.scene.ShadowMapSize[1] = float(sw), float(sh_)
    tables = _device_tables(hotpath, shadow, env, lut)
    ref, fragile = oracle.deferred_lighting(fc.scene, g.A, g.B, g.C, shadow, env, 32, 6, lut, g.hdr, w, h, want_fragile=True)
    d = to_device(g.hdr)
    hotpath.deferred_lighting(fc.scene, to_device(g.A), to_device(g.B), to_device(g.C), tables, d, w, h)
    torch.cuda.synchronize()
    nbad, worst, _ = hdr_mismatch(d.cpu().numpy().view(np.uint16), ref, exclude=fragile)
    assert nbad == 0, (case, nbad, worst)
    assert (~fragile.astype(bool)).sum() > 0.8 * w * h
    if ss is None:  # the world-space vectors must actually differ from the rigid ones: the rigid path on these inputs fails
        rigid = oracle.deferred_lighting(_rigid_copy(fc.scene), g.A, g.B, g.C, shadow, env, 32, 6, lut, g.hdr, w, h)
        assert hdr_mismatch(rigid, ref)[0] > 0


def _rigid_copy(scene):
    import copy
    from unclerenderer_amd import hostmath
    c = copy.deepcopy(scene)
    fc = hostmath.build_frame_constants("sponza", 96, 40, shadow_size=256)
    for k in range(16):
        c.ViewInverse[k] = fc.scene.ViewInverse[k]
    for k in range(3):
        c.CameraPosition[k] = fc.scene.CameraPosition[k]
    return c


# ---------------------------------------------------------------------------------------------------------------------
# full BASELINE sizes through size-independent properties
# ---------------------------------------------------------------------------------------------------------------------
def test_full_size_properties_4k(hotpath, oracle):
    from unclerenderer_amd import hostmath, synth
    from unclerenderer_amd.hotpath import HzbLayout, to_device
    torch = _torch()
    import torch.nn.functional as F
    w, h = 3840, 2160
    fc = hostmath.build_frame_constants("sponza", w, h, shadow_size=512)
    g = synth.gbuffer_iid(w, h, 3)
    # HZB: with even dims all the way down to mip 3, every mip is the 2x2 min-pool of its parent
    lay = HzbLayout(w, h)
    d_depth = to_device(g.depth)
    hzb = torch.zeros(lay.total, device="cuda")
    hotpath.build_hzb(d_depth, hzb, lay)
    parent = d_depth.view(1, 1, h, w)
    for (off, mw, mh) in lay.as_list()[:4]:
        pooled = -F.max_pool2d(-parent, 2)
        mip = hzb[off:off + mw * mh].view(1, 1, mh, mw)
        assert torch.equal(pooled, mip)
        parent = mip
    # the top of the chain is the global minimum
    off, mw, mh = lay.as_list()[-1]
    assert (mw, mh) == (1, 1)
    # odd-sized parents drop their last row/column (floor), so the 1x1 mip is >= the true minimum
    assert float(hzb[off]) >= float(d_depth.min())
    # oracle agrees on a cropped corner that includes the clamped edge
    ref = oracle.build_hzb(g.depth, lay.as_list(), lay.total)
    assert np.array_equal(hzb.cpu().numpy().view(np.uint32)[lay.mips[4].offset:], np.nan_to_num(ref, nan=0.0).view(np.uint32)[lay.mips[4].offset:])

    # lighting: 8 row bands == whole frame, and the per-band result does not depend on the band it was computed in
    shadow = synth.shadow_map_noise(512, 1)
    env = synth.env_cube_procedural(64, 7)
    lut = synth.brdf_lut_procedural(128, 32)
    fc.scene.EnvMapMipCount = 7.0
    tables = hotpath.make_tables(to_device(shadow), hotpath.stage_env_cube(env, 64, 7), 64, 7, to_device(lut))
    dA, dB, dC = to_device(g.A), to_device(g.B), to_device(g.C)
    whole = to_device(g.hdr)
    hotpath.deferred_lighting_sky(fc.scene, fc.sky, dA, dB, dC, d_depth, tables, whole, w, h)
    parts = to_device(g.hdr)
    for r in range(8):
        sl = slice(r * 270, (r + 1) * 270)
        hotpath.deferred_lighting_sky(fc.scene, fc.sky, dA[sl], dB[sl], dC[sl], d_depth[sl], tables, parts[sl], w, h, r * 270, 270)
    torch.cuda.synchronize()
    assert torch.equal(whole, parts)
    out = whole.cpu().numpy().view(np.float16).astype(np.float32)
    assert np.isfinite(out).all(), "after the sky pass no pixel may be NaN/inf"
    assert (out[..., 3][g.depth == 0] == 1.0).all() and (out[..., 3][g.depth > 0] == 2.0).all()
    # oracle on a 64-row band of the 4K frame
    r0 = 1024
    sl = slice(r0, r0 + 64)
    ref_l, frag = oracle.deferred_lighting(fc.scene, g.A[sl], g.B[sl], g.C[sl], shadow, env, 64, 7, lut, g.hdr[sl], w, h, r0, 64, want_fragile=True)
    ref = oracle.sky_atmosphere(fc.sky, g.depth[sl], ref_l, w, h, r0, 64)
    nbad, worst, _ = hdr_mismatch(whole[sl].cpu().numpy().view(np.uint16), ref, exclude=frag)
    assert nbad == 0, (nbad, worst)


def test_cull_one_million(hotpath, oracle):
    """BASELINE config 5 (scaled HZB): 1 M instances, bit-exact words + list against the oracle."""
    cnt, stats = _cull_case(hotpath, oracle, 1_000_000, True, seed=5, w=960, h=540, box=400.0)
    assert cnt > 1000 and stats[0] > 0 and stats[1] > 0


def test_tonemap_parity(hotpath, oracle):
    """Next row §8f-1: 8-bit output may differ by one LSB where exp2/log2 and powf round differently."""
    from unclerenderer_amd.hotpath import to_device
    torch = _torch()
    rng = np.random.default_rng(5)
    hdr = np.zeros((64, 257, 4), np.float16)
    hdr[..., :3] = (rng.random((64, 257, 3)) ** 3 * 6.0).astype(np.float16)
    hdr[..., 3] = 2.0
    hdr[0, :8, :3] = [[0, 0, 0], [1, 1, 1], [0.05, 0.05, 0.05], [8, 0.1, 0.1], [0.76, 0.76, 0.76], [65504, 0, 0], [0.08, 0.5, 0.9], [1e-4, 1e-5, 0]]
    bits = hdr.view(np.uint16)
    for kw in (dict(), dict(enable_tonemap=False), dict(exposure=0.9, gamma=2.2), dict(exposure=2.0, exposure_ev=-1.5)):
        ref = oracle.tonemap(bits, **kw)
        out = torch.zeros((64, 257), dtype=torch.int32, device="cuda")
        ev = torch.tensor([kw["exposure_ev"]], device="cuda") if "exposure_ev" in kw else None
        hotpath.tonemap(to_device(bits), out, 257, 64, exposure=kw.get("exposure", 1.0), gamma=kw.get("gamma", 2.2),
                        enable_tonemap=kw.get("enable_tonemap", True), exposure_ev=ev)
        got = out.cpu().numpy().view(np.uint32)
        sh = np.array([0, 8, 16, 24], np.uint32)
        d = np.abs(((got[..., None] >> sh) & 255).astype(np.int32) - ((ref[..., None] >> sh) & 255).astype(np.int32))
        assert d.max() <= 1 and (d > 0).mean() < 2e-3, (d.max(), (d > 0).mean())
        # the same pixels through the other launch forms: a band whose start is only 8-byte aligned (one pixel per lane), and
        # an odd pixel count (pixel pairs + the last pixel on its own) - bit for bit what the whole frame gave
        d_bits = to_device(bits)
        for sl in (slice(1, 64), slice(0, 63), slice(5, 6)):
            part = torch.zeros((64, 257), dtype=torch.int32, device="cuda")
            hotpath.tonemap(d_bits[sl], part[sl], 257, sl.stop - sl.start, exposure=kw.get("exposure", 1.0), gamma=kw.get("gamma", 2.2),
                            enable_tonemap=kw.get("enable_tonemap", True), exposure_ev=ev)
            assert torch.equal(part[sl], out[sl]), sl


def test_lighting_with_shipped_ibl_assets(hotpath, oracle):
    """Lighting parity with the reference's own IBL tables: output_pmrem.dds (BC6H_SF16, decoded by csrc/dds.cpp) and
    PreintegratedGF.dds, 9 mips, EnvMapMipCount = 9."""
    from pathlib import Path
    from unclerenderer_amd import assets, hostmath, synth
    from unclerenderer_amd.hotpath import to_device
    torch = _torch()
    adir = Path(__file__).parent / "golden" / "assets"
    env, base, mips, bad = assets.load_env_cube_dds(adir / "output_pmrem.dds")
    lut = assets.load_brdf_lut_dds(adir / "PreintegratedGF.dds")
    assert (base, mips, bad) == (256, 9, 0)
    w, h = 320, 180
    fc = hostmath.build_frame_constants("sponza", w, h, shadow_size=256, env_mip_count=9)
    shadow = synth.shadow_map_noise(256, 77)
    tables = hotpath.make_tables(to_device(shadow), hotpath.stage_env_cube(env, base, mips), base, mips, to_device(lut))
    for g in (synth.gbuffer_scene(fc.view, fc.proj, fc.camera_position, w, h, 77), synth.gbuffer_iid(w, h, 77)):
        lit, frag = oracle.deferred_lighting(fc.scene, g.A, g.B, g.C, shadow, env, base, mips, lut, g.hdr, w, h, want_fragile=True)
        ref = oracle.sky_atmosphere(fc.sky, g.depth, lit, w, h)
        hdr = to_device(g.hdr)
        hotpath.deferred_lighting_sky(fc.scene, fc.sky, to_device(g.A), to_device(g.B), to_device(g.C), to_device(g.depth), tables, hdr, w, h)
        torch.cuda.synchronize()
        nbad, worst, _ = hdr_mismatch(hdr.cpu().numpy().view(np.uint16), ref, exclude=frag)
        assert nbad == 0, (nbad, worst)


@pytest.mark.parametrize("scene_name,file,count", [("pica_pica", "pica_pica", 170), ("duck", "Duck", 1), ("sponza", "sponza", 25)])
def test_cull_on_shipped_scene_bounds(hotpath, oracle, scene_name, file, count):
    """BASELINE configs 1/3/4: the cull over the scenes' real draw-command AABBs (csrc/scene.cpp extraction), HZB from a
    synthetic depth through the scene's own camera."""
    from pathlib import Path
    from unclerenderer_amd import hostmath, scene, synth
    from unclerenderer_amd.hotpath import HzbLayout, to_device
    torch = _torch()
    sb = scene.load_scene_bounds(Path(__file__).parent / "golden" / "assets" / "Scenes" / f"{file}.json")
    assert sb.count == count
    w, h = 512, 288
    fc = hostmath.build_frame_constants(scene_name, w, h)
    depth = (synth.hash_unit(9, *synth._grid(w, 0, h), 0) * np.float32(0.004)).astype(np.float32)  # far-ish random depth: some boxes hide, some do not
    lay = HzbLayout(w, h)
    hzb = np.nan_to_num(oracle.build_hzb(depth, lay.as_list(), lay.total))
    for hzb_on in (False, True):
        consts = hostmath.pack_culling_constants(fc.view, fc.proj, count, hzb_on, lay.count, lay.width, lay.height, True)
        args0 = synth.indirect_args_initial(count)
        ref_args, ref_stats, ref_vis, ref_cnt = oracle.cull_indirect_args(consts, sb.bounds, hzb, lay.as_list(), args0)
        d_args, d_stats = to_device(args0), torch.zeros(2, dtype=torch.int32, device="cuda")
        d_vis, d_cnt = torch.zeros(count, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
        hotpath.cull_indirect_args(consts, to_device(sb.bounds), to_device(hzb), lay, d_args, d_stats, d_vis, d_cnt)
        assert np.array_equal(d_args.cpu().numpy().view(np.uint32), ref_args)
        assert int(d_cnt.cpu()[0]) == ref_cnt and np.array_equal(d_vis.cpu().numpy().view(np.uint32)[:ref_cnt], ref_vis)
        assert np.array_equal(d_stats.cpu().numpy().view(np.uint32), ref_stats)
    if scene_name == "pica_pica":
        assert 0 < ref_cnt <= count


@pytest.mark.parametrize("w,h", [(64, 8), (67, 13), (320, 180), (1, 1), (130, 3), (513, 17), (1030, 9), (255, 8), (2, 40)])
def test_temporal_aa_bit_exact(hotpath, oracle, w, h):
    """Next row §8f-4: 3x3 clamp + blend (64-column x 8-row register strips; without history a copy), whole frame and 3
    uneven row bands, bit for bit."""
    from unclerenderer_amd.hotpath import to_device
    torch = _torch()
    rng = np.random.default_rng(w * 31 + h)
    cur = (rng.random((h, w, 4)) ** 2 * 8).astype(np.float16)
    hist = (rng.random((h, w, 4)) ** 2 * 8).astype(np.float16)
    cur[..., 3] = 2.0
    cb, hb = cur.view(np.uint16), hist.view(np.uint16)
    d_cur, d_hist = to_device(cb), to_device(hb)
    for use, wt in ((True, 0.9), (True, 0.35), (False, 0.9)):
        ref = oracle.temporal_aa(cb, hb, wt, use)
        out = torch.zeros((h, w, 4), dtype=torch.int16, device="cuda")
        hotpath.temporal_aa(d_cur, d_hist, out, wt, use, w, h)
        assert np.array_equal(out.cpu().numpy().view(np.uint16), ref)
        parts = torch.zeros((h, w, 4), dtype=torch.int16, device="cuda")
        cuts = sorted({0, h // 3, (2 * h) // 3 + (1 if h > 2 else 0), h})
        for a, b in zip(cuts, cuts[1:]):
            if b > a:
                hotpath.temporal_aa(d_cur, d_hist[a:b], parts[a:b], wt, use, w, h, a, b - a)
        assert torch.equal(parts, out)


def test_cull_more_than_4096_blocks(hotpath, oracle):
    """1.3 M instances = 5079 blocks of 256: the compaction's prefix over the block counts keeps sixteen loads per thread in flight for
    the first 4096 blocks and loops over the rest (csrc/cull.hip: compact_kernel); words, list, count and counters bit-exact."""
    from unclerenderer_amd import hostmath, synth
    from unclerenderer_amd.hotpath import HzbLayout, to_device
    torch = _torch()
    w, h, n = 512, 288, 1_300_000
    fc = hostmath.build_frame_constants("sponza", w, h)
    depth = (synth.hash_unit(11, *synth._grid(w, 0, h), 0) * np.float32(0.004)).astype(np.float32)
    lay = HzbLayout(w, h)
    hzb = np.nan_to_num(oracle.build_hzb(depth, lay.as_list(), lay.total))
    bounds = synth.instances_random(n, 11, center=fc.camera_position, box=300.0)
    consts = hostmath.pack_culling_constants(fc.view, fc.proj, n, True, lay.count, lay.width, lay.height, True)
    args0 = synth.indirect_args_initial(n)
    ref_args, ref_stats, ref_vis, ref_cnt = oracle.cull_indirect_args(consts, bounds, hzb, lay.as_list(), args0)
    d_args, d_stats = to_device(args0), torch.zeros(2, dtype=torch.int32, device="cuda")
    d_vis, d_cnt = torch.full((n,), -1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    hotpath.cull_indirect_args(consts, to_device(bounds), to_device(hzb), lay, d_args, d_stats, d_vis, d_cnt)
    torch.cuda.synchronize()
    assert np.array_equal(d_args.cpu().numpy().view(np.uint32), ref_args)
    assert int(d_cnt.cpu()[0]) == ref_cnt and ref_cnt > 4096
    assert np.array_equal(d_vis.cpu().numpy().view(np.uint32)[:ref_cnt], ref_vis)
    assert np.array_equal(d_stats.cpu().numpy().view(np.uint32), ref_stats)


def test_lighting_view_ray_along_the_light(hotpath, oracle):
    """A camera that looks straight into the light: around the frame's centre V.L -> -1 and |V + L|^2 = 2 + 2 V.L cancels (the
    streaming kernel's algebraic half vector loses 1e-7 / (1 + V.L) of relative accuracy there). The G-buffer is crafted so that
    those pixels are lit, face the viewer, and have N.H ~ 0.7 at low roughness: a specular term that is large and well conditioned
    in |V + L| itself. Both kernels must sit on the oracle like everywhere else; the streaming kernel's waves with such a pixel take
    |V + L| from the components (csrc/lighting.hip), and the test checks that pixels with 1 + V.L < 1e-3 are really in the frame."""
    import dataclasses
    from unclerenderer_amd import hostmath, lib, synth
    from unclerenderer_amd.hotpath import to_device
    torch = _torch()
    w, h = 320, 180
    base = hostmath.SCENES["sponza"]
    L = hostmath.build_frame_constants(base, w, h, shadow_size=256).light_direction.astype(np.float64)
    pos = np.array(base.camera_position, np.float64)
    preset = dataclasses.replace(base, camera_rotation_deg=None, camera_look_at=tuple(pos + 10.0 * L), light_intensity=3.0)
    fc = hostmath.build_frame_constants(preset, w, h, shadow_size=256, env_mip_count=6)
    P = np.asarray(fc.proj, np.float32).reshape(4, 4)
    V4 = np.asarray(fc.view, np.float32).reshape(4, 4)
    Lv = (L.astype(np.float32) @ V4[:3, :3]).astype(np.float64)  # light direction in view space: ~(0, 0, 1)
    assert Lv[2] > 0.999999
    xs, ys = np.meshgrid(np.arange(w, dtype=np.float64) + 0.5, np.arange(h, dtype=np.float64) + 0.5)
    a, b = (xs / w * 2 - 1) / P[0, 0], -(ys / h * 2 - 1) / P[1, 1]
    n = np.sqrt(a * a + b * b + 1.0)
    one_plus_vl = 1.0 - (a * Lv[0] + b * Lv[1] + Lv[2]) / n  # V = -(a, b, 1) / n
    assert (one_plus_vl < 1e-3).sum() > 100 and (one_plus_vl < 1e-4).sum() > 10
    r = np.maximum(np.sqrt(a * a + b * b), 1e-9)
    t2 = np.stack([-a / r, -b / r, np.zeros_like(r)], -1)   # towards the frame's centre: N.V > 0 needs a component along it
    t1 = np.stack([b / r, -a / r, np.zeros_like(r)], -1)    # across
    eps = 0.3 * 0.7 * r                                      # N.L = eps > 0, N.V ~ 0.7 * 0.7 r / n > 0, N.H ~ 0.7
    N = 0.7 * t1 + 0.7 * t2 + eps[..., None] * np.array([0.0, 0.0, 1.0])
    N /= np.linalg.norm(N, axis=-1, keepdims=True)
    view_z = np.full((h, w), 5.0)
    A = np.concatenate([N, -view_z[..., None]], -1).astype(np.float16).view(np.uint16)
    rough = 0.08 + 0.2 * synth.hash_unit(77, *synth._grid(w, 0, h), 0)
    B = np.stack([np.full((h, w), 0.04), np.zeros((h, w)), rough, np.ones((h, w))], -1).astype(np.float16).view(np.uint16)
    Cc = np.full((h, w), 0xFF909090, np.uint32)
    hdr = np.zeros((h, w, 4), np.float16); hdr[..., 3] = 1.0
    hdr = hdr.view(np.uint16)
    shadow = np.ones((256, 256), np.float32)  # nothing in shadow: the direct term is what is being looked at
    env = synth.env_cube_procedural(32, 6)
    lut = synth.brdf_lut_procedural(128, 32)
    tables = _device_tables(hotpath, shadow, env, lut)
    ref, fragile = oracle.deferred_lighting(fc.scene, A, B, Cc, shadow, env, 32, 6, lut, hdr, w, h, want_fragile=True)
    reff = ref.view(np.float16).astype(np.float32)
    near = one_plus_vl < 1e-3
    assert np.isfinite(reff[near]).all() and reff[near][..., :3].max() > 0.05, "the direct specular term must be visible where V.L -> -1"
    try:
        for name, stream in (("streaming", 1), ("per-tile", 0)):
            hotpath.set_option(lib.UR_OPT_LIGHTING_STREAM, stream)
            d = to_device(hdr)
            hotpath.deferred_lighting(fc.scene, to_device(A), to_device(B), to_device(Cc), tables, d, w, h)
            torch.cuda.synchronize()
            nbad, worst, where = hdr_mismatch(d.cpu().numpy().view(np.uint16), ref, exclude=fragile)
            assert nbad == 0, (name, nbad, worst, int((where & near).sum()))
    finally:
        hotpath.set_option(lib.UR_OPT_LIGHTING_STREAM, 1)
    assert fragile.mean() < 0.02


def test_env_cube_layout_tag_is_checked(hotpath):
    """ur_lighting_tables.env_cube_texels carries the staged layout's size: a buffer sized for another layout (round 2 staged the
    bordered faces only) is refused, not read out of bounds."""
    from unclerenderer_amd import lib
    from unclerenderer_amd.hotpath import to_device
    w, h = 64, 16
    fc, g, shadow, env, lut = _lighting_inputs("sponza", w, h, seed=3, mode="scene")
    tables = _device_tables(hotpath, shadow, env, lut)
    good = tables.env_cube_texels
    assert good == lib.load().ur_env_cube_texels(32, 6)
    bordered_only = sum(6 * (max(1, 32 >> m) + 2) ** 2 for m in range(6))
    for bad in (0, bordered_only, good + 1):
        tables.env_cube_texels = bad
        with pytest.raises(lib.UrError) as e:
            hotpath.deferred_lighting(fc.scene, to_device(g.A), to_device(g.B), to_device(g.C), tables, to_device(g.hdr), w, h)
        assert e.value.code == lib.UR_EINVAL and "another layout" in str(e.value)
    tables.env_cube_texels = good
    hotpath.deferred_lighting(fc.scene, to_device(g.A), to_device(g.B), to_device(g.C), tables, to_device(g.hdr), w, h)
