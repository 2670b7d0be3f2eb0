"""Footprints of DeferredLighting, SkyAtmosphere and the fused launch (csrc/lighting.hip, csrc/lighting_tiled.hip) under the rules of tests/footprint.py: both
kernels, the twelve-wave workgroups, a balanced schedule, shadow maps down to 1x1, every irradiance table form, shapes whose last
tile row hangs over the band, bands, one 4K frame; G-buffer A/B/C, depth, shadow map, staged cube and BRDF LUT each between poisoned
guards, the HDR target between hashed ones. Nothing here judges a value."""
import numpy as np
import pytest

from tests import footprint as F

pytestmark = pytest.mark.gpu


def _inputs(w, h, seed, shadow_size=256, shadow_strength=1.0, mode="scene"):
    from tests.test_gpu_parity import _lighting_inputs
    return _lighting_inputs("sponza", w, h, seed=seed, mode=mode, shadow_size=shadow_size, shadow_strength=shadow_strength)


def _staged(hotpath, env, base, mips):
    import torch
    t = hotpath.stage_env_cube(env, base, mips)
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint16)


def _run(hotpath, fc, g, shadow, cube, lut, w, h, row0, rows, kinds=("lighting", "sky", "fused"), base=32, mips=6, what=""):
    """The three entry points on rows [row0, row0 + rows) of the w x h frame g, every table guarded."""
    sl = slice(row0, row0 + rows)
    ins = {"A": g.A[sl], "B": g.B[sl], "C": g.C[sl], "D": g.depth[sl], "shadow": shadow, "cube": cube, "lut": lut}

    def tables(b):
        return hotpath.make_tables(b["shadow"], b["cube"], base, mips, b["lut"])

    calls = {"lighting": lambda b: hotpath.deferred_lighting(fc.scene, b["A"], b["B"], b["C"], tables(b), b["hdr"], w, h, row0, rows),
             "sky": lambda b: hotpath.sky_atmosphere(fc.sky, b["D"], b["hdr"], w, h, row0, rows),
             "fused": lambda b: hotpath.deferred_lighting_sky(fc.scene, fc.sky, b["A"], b["B"], b["C"], b["D"], tables(b), b["hdr"], w, h, row0, rows)}
    out = {}
    for k in kinds:
        out[k] = F.run_rules(calls[k], ins, {"hdr": g.hdr[sl]}, row_bytes={"cube": 8 * (base + 2), "lut": lut.shape[1] * 4},
                             what=f"{k} {w}x{h} rows {row0}+{rows} {what}")["hdr"]
    return out


SHAPES = [(16, 1), (48, 7), (130, 3), (272, 33), (1, 1)]


@pytest.mark.parametrize("stream", [1, 0])
@pytest.mark.parametrize("w,rows", SHAPES)
def test_lighting_shapes_footprint(hotpath, w, rows, stream):
    """ur_deferred_lighting, ur_sky_atmosphere and ur_deferred_lighting_sky under UR_OPT_LIGHTING_STREAM 1 and 0, at shapes whose 16x4
    tiles do not divide the band."""
    from unclerenderer_amd import lib
    fc, g, shadow, env, lut = _inputs(w, rows, 3)
    cube = _staged(hotpath, env, 32, 6)
    hotpath.set_option(lib.UR_OPT_LIGHTING_STREAM, stream)
    try:
        _run(hotpath, fc, g, shadow, cube, lut, w, rows, 0, rows, what=f"stream {stream}")
    finally:
        hotpath.set_option(lib.UR_OPT_LIGHTING_STREAM, 1)


@pytest.mark.parametrize("w,h,row0,rows", [(320, 270, 135, 34), (1920, 1080, 810, 270)])
def test_lighting_bands_footprint(hotpath, w, h, row0, rows):
    """ur_deferred_lighting_sky and ur_deferred_lighting on a band in the middle of a frame, both kernels."""
    from unclerenderer_amd import lib
    fc, g, shadow, env, lut = _inputs(w, h, 4)
    cube = _staged(hotpath, env, 32, 6)
    try:
        for stream in (1, 0):
            hotpath.set_option(lib.UR_OPT_LIGHTING_STREAM, stream)
            _run(hotpath, fc, g, shadow, cube, lut, w, h, row0, rows, kinds=("lighting", "fused"), what=f"stream {stream}")
    finally:
        hotpath.set_option(lib.UR_OPT_LIGHTING_STREAM, 1)


def test_lighting_twelve_waves_and_balance_footprint(hotpath):
    """ur_deferred_lighting_sky with UR_OPT_LIGHTING_WAVES_PER_WG = 12 at a shape with a partial tile row, and with a balanced schedule
    (ur_debug_lighting_schedule shows a run-time part) at the pools and chunks of tests/test_gpu_balance.py."""
    from unclerenderer_amd import lib
    try:
        hotpath.set_option(lib.UR_OPT_LIGHTING_WAVES_PER_WG, 12)
        for (w, h) in ((272, 33), (320, 180)):
            fc, g, shadow, env, lut = _inputs(w, h, 5)
            _run(hotpath, fc, g, shadow, _staged(hotpath, env, 32, 6), lut, w, h, 0, h, kinds=("lighting", "fused"), what="12 waves")
        hotpath.set_option(lib.UR_OPT_LIGHTING_WAVES_PER_WG, 16)
        for (w, h, pool, chunk) in ((1920, 1080, 3, 2), (1920, 1083, 6, 3)):
            fc, g, shadow, env, lut = _inputs(w, h, 6)
            hotpath.set_option(lib.UR_OPT_LIGHTING_BALANCE, 1)
            hotpath.set_option(lib.UR_OPT_BALANCE_POOL_16THS, pool)
            hotpath.set_option(lib.UR_OPT_BALANCE_CHUNK_SHIFT, chunk)
            _run(hotpath, fc, g, shadow, _staged(hotpath, env, 32, 6), lut, w, h, 0, h, kinds=("fused",), what=f"pool {pool} chunk {chunk}")
            sched = hotpath.lighting_schedule()
            assert sched["pool_chunks"] > 0 and sched["static_tiles"] < sched["tiles"], sched
        hotpath.flush()
    finally:
        hotpath.set_option(lib.UR_OPT_LIGHTING_WAVES_PER_WG, 16)
        hotpath.set_option(lib.UR_OPT_LIGHTING_BALANCE, 1)
        hotpath.set_option(lib.UR_OPT_BALANCE_POOL_16THS, 3)
        hotpath.set_option(lib.UR_OPT_BALANCE_CHUNK_SHIFT, 4)


@pytest.mark.parametrize("sx,sy", [(0, 0), (1, 1), (2, 5), (8, 8)])
def test_lighting_shadow_maps_footprint(hotpath, sx, sy):
    """ur_deferred_lighting and ur_deferred_lighting_sky without shadows (shadow_map NULL) and with shadow maps of 1x1, 2x5 and 8x8
    texels, whose bilinear taps all touch the border."""
    w, h = 272, 33
    fc, g, _, env, lut = _inputs(w, h, 7, shadow_size=8, shadow_strength=1.0 if sx else 0.0)
    shadow = None
    if sx:
        fc.scene.ShadowMapSize[0], fc.scene.ShadowMapSize[1] = float(sx), float(sy)
        shadow = np.random.default_rng(sx * 10 + sy).random((sy, sx), dtype=np.float32)
    _run(hotpath, fc, g, shadow, _staged(hotpath, env, 32, 6), lut, w, h, 0, h, kinds=("lighting", "fused"), what=f"shadow {sx}x{sy}")


@pytest.mark.parametrize("shadows", [False, True])
@pytest.mark.parametrize("env_mip_count", [3, 5, 6])
def test_lighting_irradiance_forms_footprint(hotpath, env_mip_count, shadows):
    """ur_deferred_lighting and ur_deferred_lighting_sky with the irradiance mip 8x8 (gathered from memory), 2x2 and 1x1 (LDS tables), as
    tests/test_gpu_configs.py::test_every_irradiance_table_form."""
    from unclerenderer_amd import hostmath, synth
    w, h = 320, 180
    fc = hostmath.build_frame_constants("sponza", w, h, shadow_size=256, shadow_strength=1.0 if shadows else 0.0, env_mip_count=env_mip_count)
    env, lut = synth.env_cube_procedural(32, 6), synth.brdf_lut_procedural(128, 32)
    shadow = synth.shadow_map_noise(256, 41) if shadows else None
    g = synth.gbuffer_scene(fc.view, fc.proj, fc.camera_position, w, h, 41)
    _run(hotpath, fc, g, shadow, _staged(hotpath, env, 32, 6), lut, w, h, 0, h, kinds=("lighting", "fused"), what=f"mips {env_mip_count}")


def test_lighting_4k_footprint(hotpath):
    """ur_deferred_lighting_sky on one whole 3840 x 2160 frame."""
    w, h = 3840, 2160
    fc, g, shadow, env, lut = _inputs(w, h, 8, mode="iid")
    _run(hotpath, fc, g, shadow, _staged(hotpath, env, 32, 6), lut, w, h, 0, h, kinds=("fused",), what="4K")


@pytest.mark.parametrize("base,mips", [(32, 6), (16, 5), (4, 3), (1, 1)])
def test_stage_env_cube_footprint(hotpath, base, mips):
    """ur_stage_env_cube: the output is exactly ur_env_cube_texels(base, mips) units, every one of them inside the guards."""
    import ctypes as C

    import torch
    from unclerenderer_amd import lib, synth
    env = np.ascontiguousarray(synth.env_cube_procedural(base, mips), np.uint16)
    n = int(hotpath._L.ur_env_cube_texels(base, mips))
    assert n > 0
    outs = []
    for seed in (1, 2):
        dst = F.guarded(np.zeros((n, 4), np.uint16), "cuda", ("hash", seed), row_bytes=8 * (base + 2))
        lib.check(hotpath._L.ur_stage_env_cube(hotpath.ctx, env.ctypes.data_as(C.c_void_p), base, mips, C.c_void_p(dst.data_ptr())), "ur_stage_env_cube")
        torch.cuda.synchronize()
        r = F.check(dst)
        assert r.ok, f"stage_env_cube {base}/{mips}: {r}"
        outs.append(F.host_bytes(dst))
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], F.host_bytes(hotpath.stage_env_cube(env, base, mips)))


def test_stream_ceiling_and_timeline_footprint(hotpath):
    """ur_debug_stream_ceiling (four inputs, one output of exactly elements16 * 16 bytes) and ur_debug_timeline (capacity_pairs pairs:
    launches beyond the capacity write nothing)."""
    import torch
    from unclerenderer_amd import hostmath
    rng = np.random.default_rng(9)
    for n16 in (1, 63, 4097, 1 << 16):
        ins = {f"in{i}": rng.random((n16, 4), dtype=np.float32) for i in range(4)}
        F.run_rules(lambda b: hotpath.stream_ceiling([b["in0"], b["in1"], b["in2"], b["in3"]], b["out"]), ins,
                    {"out": rng.random((n16, 4), dtype=np.float32)}, aligns={k: 16 for k in ("in0", "in1", "in2", "in3", "out")},
                    what=f"stream_ceiling {n16}")
    fc = hostmath.build_frame_constants("sponza", 640, 360)
    n = 300
    from unclerenderer_amd import synth
    from unclerenderer_amd.hotpath import to_device
    bounds = to_device(synth.instances_random(n, 1, center=fc.camera_position, box=60.0))
    consts = hostmath.pack_culling_constants(fc.view, fc.proj, n, False, 0, 0, 0, False)
    pairs0 = np.tile(np.array([[-1, 0]], np.int64), (2, 1))
    pairs = F.guarded(pairs0, "cuda", ("hash", 4), align=8)
    hotpath.debug_timeline(pairs)
    try:
        for _ in range(4):  # four launches, two pairs
            hotpath.cull_indirect_args(consts, bounds, None, None, to_device(synth.indirect_args_initial(n)))
        torch.cuda.synchronize()
    finally:
        hotpath.debug_timeline(None)
    r = F.check(pairs)
    assert r.ok, f"debug_timeline: {r}"
    got = pairs.cpu().numpy()
    assert (got[:, 0] != -1).all() and (got[:, 1] >= got[:, 0]).all(), got


def test_detector_lighting_reads_past_its_input(hotpath):
    """The read rule bites: Lighting told rows + 1 on a G-buffer whose last row lies in the guard shades that row from the guard's bytes,
    so the "ones" and "zeros" runs differ in it (and only in it). The HDR target has rows + 1 real rows: nothing is written outside."""
    import torch
    w, rows = 272, 8
    fc, g, shadow, env, lut = _inputs(w, rows + 1, 10)
    tables = hotpath.make_tables(F.plain(shadow, "cuda"), hotpath.stage_env_cube(env, 32, 6), 32, 6, F.plain(lut, "cuda"))
    B, Cc = F.plain(g.B, "cuda"), F.plain(g.C, "cuda")
    out = {}
    for poison in ("ones", "zeros"):
        A = F.guarded(g.A[:rows], "cuda", poison)  # one row short: row `rows` is the first row of the guard
        hdr = F.guarded(g.hdr, "cuda", ("hash", 5))
        hotpath.deferred_lighting(fc.scene, A, B, Cc, tables, hdr, w, rows + 1, 0, rows + 1)
        torch.cuda.synchronize()
        assert F.check(hdr).ok and F.check(A).ok
        out[poison] = F.host_bytes(hdr).reshape(rows + 1, -1)
    assert np.array_equal(out["ones"][:rows], out["zeros"][:rows])
    assert not np.array_equal(out["ones"][rows], out["zeros"][rows]), "a value from outside the input reached the output unseen"
