"""Footprints of GpuDebugPrint (csrc/debug_print.hip), the row all-gather and the whole frame (csrc/frame/) under the
rules of tests/footprint.py: every resource a frame is given sits between guards, over two frames so that the HZB, the luminance pair
and the TemporalAA history are live. Nothing here judges a value."""
import ctypes as C

import numpy as np
import pytest

from tests import footprint as F

pytestmark = pytest.mark.gpu


def _ldr(h, w, seed):
    return np.random.default_rng(seed).integers(0, 2 ** 32, (h, w), dtype=np.uint32)


@pytest.mark.parametrize("w,h,row0,rows", [(200, 120, 40, 33), (64, 64, 0, 64), (1920, 1080, 405, 270)])
def test_debug_print_footprint(hotpath, w, h, row0, rows):
    """ur_debug_print_reset, ur_debug_print_stats, ur_debug_print_text and ur_debug_print_draw on a buffer of exactly
    ur_debug_print_buffer_bytes(): the draw composites on a band in the middle of a taller LDR image whose other rows keep their bytes;
    text sits on the band's first and last row and at columns 0 and w - 1; the font atlas and the glyph table are guarded inputs."""
    from tests import debug_print_cases as K
    from unclerenderer_amd.hotpath import debug_print_buffer_bytes
    atlas, glyphs, first, count = K.builtin_font()
    nb = debug_print_buffer_bytes()
    assert nb == 4 + 4096 * 16
    rng = np.random.default_rng(w)
    outside = np.ones((h, w), bool)
    outside[row0:row0 + rows] = False

    def call(b):
        hotpath.debug_print_reset(b["buffer"], b["stats_out"])
        hotpath.debug_print_stats(b["stats_in"], b["buffer"])
        for (x, y) in ((0, row0), (w - 1, row0), (0, row0 + rows - 1), (w - 1, row0 + rows - 1), (w // 2, row0 + rows // 2), (3, max(row0 - 4, 0)),
                       (5, min(row0 + rows + 2, h - 1))):
            hotpath.debug_print_text(b["buffer"], x, y, b"EDGE 0189", 0xC0FF8040)
        hotpath.debug_print_draw(b["buffer"], b["glyphs"], b["atlas"], b["ldr"][row0:row0 + rows], w, h, row0, rows, first_char=first,
                                 char_count=count)

    base = F.run_rules(call, {"stats_in": np.array([2718, 31415], np.uint32), "glyphs": np.ascontiguousarray(glyphs, np.float32),
                              "atlas": np.ascontiguousarray(atlas, np.uint8)},
                       {"buffer": rng.integers(0, 2 ** 32, nb // 4, dtype=np.uint32), "stats_out": np.array([7, 7], np.uint32), "ldr": _ldr(h, w, 1)},
                       aligns={"buffer": 4, "stats_in": 4, "stats_out": 4, "glyphs": 4, "atlas": 4}, row_bytes={"buffer": 16},
                       untouched=lambda r: {"ldr": outside, "buffer": np.arange(nb // 4) >= 1 + 4 * min(int(r["buffer"][0]), 4096)},
                       what=f"debug_print {w}x{h} rows {row0}+{rows}")
    assert base["stats_out"].tolist() == [0, 0] and 60 < int(base["buffer"][0]) < 4096
    assert (base["ldr"][row0:row0 + rows] != _ldr(h, w, 1)[row0:row0 + rows]).any(), "the band must be drawn on"


def test_allgather_rows_footprint(hotpath):
    """ur_allgather_rows, ur_allgather_rows_bytes and ur_allgather_rows_bytes_ex on a one-rank communicator: the in-place gather of a
    guarded image leaves the image and its guards as they are."""
    import torch
    from tests.test_gpu_rccl import _rccl, _UniqueId
    from unclerenderer_amd import lib
    L = lib.load()
    rccl = _rccl()
    rccl.ncclGetUniqueId.argtypes = [C.POINTER(_UniqueId)]
    rccl.ncclCommInitRank.argtypes = [C.POINTER(C.c_void_p), C.c_int, _UniqueId, C.c_int]
    rccl.ncclCommDestroy.argtypes = [C.c_void_p]
    uid = _UniqueId()
    assert rccl.ncclGetUniqueId(C.byref(uid)) == 0
    comm = C.c_void_p()
    torch.cuda.set_device(0)
    assert rccl.ncclCommInitRank(C.byref(comm), 1, uid, 0) == 0 and comm.value
    try:
        w, h = 250, 63
        rng = np.random.default_rng(3)
        hdr0, ldr0 = rng.integers(0, 2 ** 16, (h, w, 4), dtype=np.uint16), _ldr(h, w, 4)
        hdr, ldr = F.guarded(hdr0, "cuda", ("hash", 1)), F.guarded(ldr0, "cuda", ("hash", 2))
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        assert L.ur_allgather_rows(hotpath.ctx, comm, p(hdr), w, h, 1, 0) == lib.UR_OK, L.ur_last_error()
        assert L.ur_allgather_rows_bytes(hotpath.ctx, comm, p(ldr), w * 4, h, 1, 0) == lib.UR_OK, L.ur_last_error()
        for mode in (0, 1):
            assert L.ur_allgather_rows_bytes_ex(hotpath.ctx, comm, p(ldr), w * 4, h, 1, 0, mode) == lib.UR_OK, L.ur_last_error()
        torch.cuda.synchronize()
        for t, want in ((hdr, hdr0), (ldr, ldr0)):
            r = F.check(t)
            assert r.ok, str(r)
            assert np.array_equal(F.host_bytes(t), want.view(np.uint8).reshape(-1))
    finally:
        rccl.ncclCommDestroy(comm)


def _flag_sets():
    from unclerenderer_amd import lib as u
    base = u.UR_FRAME_DEFAULT
    post = u.UR_FRAME_TONEMAP | u.UR_FRAME_TAA | u.UR_FRAME_AUTO_EXPOSURE | u.UR_FRAME_CAS | u.UR_FRAME_DEBUG_PRINT
    return {"default": base,
            "fused": base | u.UR_FRAME_FUSE_LIGHTING_SKY | u.UR_FRAME_HZB_WITH_LIGHTING,
            "post": base | post,
            "post_fused": base | post | u.UR_FRAME_FUSE_LIGHTING_SKY | u.UR_FRAME_FUSE_TONEMAP_CAS,
            "post_fused_taa": base | post | u.UR_FRAME_FUSE_LIGHTING_SKY | u.UR_FRAME_FUSE_TAA_TONEMAP,  # (the two post fusions exclude each other)
            "async": base | u.UR_FRAME_ASYNC_COMPUTE | u.UR_FRAME_CULL_VIEWS,
            "exchange": base | u.UR_FRAME_FUSE_LIGHTING_SKY | u.UR_FRAME_TONEMAP | u.UR_FRAME_TAA | u.UR_FRAME_AUTO_EXPOSURE | u.UR_FRAME_CAS
            | u.UR_FRAME_POST_EXCHANGE | u.UR_FRAME_TAA_BAND}


CASES = [(128, 72, k) for k in ("default", "fused", "post", "post_fused", "post_fused_taa", "async", "exchange")] + [(1920, 1080, "default"), (1920, 1080, "post_fused")]


@pytest.mark.parametrize("w,h,name", CASES, ids=[f"{w}x{h}-{k}" for w, h, k in CASES])
def test_frame_footprint(hotpath, w, h, name):
    """Two frames through ur_frame_render with every resource of ur_frame_resources, ur_frame_set_post, _set_taa, _set_draw_ranges,
    _set_cull_views, _set_debug_print and the two record pairs guarded."""
    from tests import debug_print_cases as K
    from unclerenderer_amd import hostmath, synth
    from unclerenderer_amd.hotpath import Frame, HzbLayout, debug_print_buffer_bytes, post_record_bytes, taa_record_bytes
    flags = _flag_sets()[name]
    n = 600
    fc = hostmath.build_frame_constants("sponza", w, h, shadow_size=128, env_mip_count=5)
    g = synth.gbuffer_scene(fc.view, fc.proj, fc.camera_position, w, h, 31)
    shadow, env, lut = synth.shadow_map_noise(128, 31), synth.env_cube_procedural(16, 5), synth.brdf_lut_procedural(128, 32)
    import torch
    cube = hotpath.stage_env_cube(env, 16, 5)
    torch.cuda.synchronize()
    cube = cube.cpu().numpy().view(np.uint16)
    lay = HzbLayout(w, h)
    bounds = synth.instances_random(n, 31, center=fc.camera_position, box=60.0)
    consts = hostmath.pack_culling_constants(fc.view, fc.proj, 0, False, 0, 0, 0, True)
    atlas, glyphs, first, count = K.builtin_font()
    planes = hostmath.frustum_planes(hostmath.light_view_projection(fc.scene_center, fc.scene_radius * 0.25, fc.light_direction))
    offsets = np.array([0, n // 3, n // 2, n], np.uint32)
    rng = np.random.default_rng(h)
    u32 = lambda *shape: rng.integers(0, 2 ** 32, shape, dtype=np.uint32)  # noqa: E731
    words = (n + 31) // 32
    PB, TB = post_record_bytes(w), taa_record_bytes(w)
    ins = {"A": g.A, "B": g.B, "C": g.C, "D": g.depth, "shadow": shadow, "cube": cube, "lut": lut, "bounds": bounds, "offsets": offsets,
           "glyphs": np.ascontiguousarray(glyphs, np.float32), "atlas": np.ascontiguousarray(atlas, np.uint8)}
    outs = {"hdr1": g.hdr, "hdr2": g.hdr, "hzb": np.zeros(lay.total, np.float32), "args": synth.indirect_args_initial(n), "stats": np.zeros(2, np.uint32),
            "vis": u32(n), "cnt": u32(1), "ldr": u32(h, w), "scratch": u32(h, w), "lum0": np.array([np.nan], np.float32),
            "lum1": np.array([np.nan], np.float32), "ring0": u32(h, w, 2).view(np.uint16).reshape(h, w, 4), "ring1": u32(h, w, 2).view(np.uint16).reshape(h, w, 4),
            "ring2": u32(h, w, 2).view(np.uint16).reshape(h, w, 4), "cmds": u32(n, 16), "counts": u32(3), "vmask": u32(words), "vcmds": u32(n, 16),
            "vcounts": u32(3), "dbg": np.zeros(debug_print_buffer_bytes() // 4, np.uint32), "post_rec": np.zeros(PB, np.uint8), "taa_rec": np.zeros(TB, np.uint8)}
    exchange = name == "exchange"

    def call(b):
        frame = Frame(hotpath)
        try:
            tables = hotpath.make_tables(b["shadow"], b["cube"], 16, 5, b["lut"])
            frame.set_post(luminance=(b["lum0"], b["lum1"]), tonemap_scratch=b["scratch"], delta_time=1 / 60)
            frame.set_taa([b["ring0"], b["ring1"], b["ring2"]], 0.9)
            frame.set_draw_ranges(b["offsets"], b["cmds"], b["counts"])
            frame.set_cull_views([dict(planes=planes, mask=b["vmask"], draw_offsets=b["offsets"], draw_commands=b["vcmds"], draw_counts=b["vcounts"])])
            frame.set_debug_print(b["dbg"], b["glyphs"], b["atlas"], first, count)
            if exchange:
                frame.set_post_records(b["post_rec"], b["post_rec"])
                frame.set_taa_records(b["taa_rec"], b["taa_rec"])
            for k in (1, 2):
                res = Frame.resources(w, h, 0, h, b["A"], b["B"], b["C"], b["D"], b[f"hdr{k}"], b["D"], b["hzb"], lay, tables, b["bounds"], b["args"], n, 0,
                                      b["vis"], b["cnt"], b["stats"], tonemap_band=b["ldr"])
                frame.render(res, consts, fc.scene, fc.sky, flags)
                if exchange:
                    frame.finish_post()
                frame.join_async()
            assert frame.hzb_ready
        finally:
            import torch
            torch.cuda.synchronize()
            frame.close()

    F.run_rules(call, ins, outs, aligns={"args": 16, "cmds": 16, "vcmds": 16, "stats": 4, "cnt": 4, "lum0": 4, "lum1": 4, "dbg": 4, "counts": 4, "vcounts": 4,
                                         "vmask": 4, "offsets": 4, "post_rec": 16, "taa_rec": 16},
                row_bytes={"hzb": lay.width * 4, "cube": 8 * 18, "dbg": 16}, what=f"frame {w}x{h} {name}")
