"""The geometry-fed frame on row bands, in one process: cull -> ShadowMap -> DepthPrepass -> GBuffer -> Build HZB -> Lighting -> Sky over the
textured 257 x 130 soup (18 draws, materials with keys 0-15), once on the whole frame and once per band of three splits - 2 x 65 (an odd
row0), 5 x 26 and the unequal (0, 37), (37, 41), (78, 52). A band frame renders the whole depth, the whole shadow map and the whole HZB
but only its rows of the G-buffer and of the HDR target; its depth_band is a window into its depth_full. Every byte a band frame leaves
equals the whole frame's, and the whole frame's equal the direct calls' and the restatement's (tests/gbuffer_tex_ref.py).
tests/test_gbuffer_tex_ref.py::test_band_seam_conditions says what the seams cut through.

UR_FRAME_CULL_VIEWS is set beside the flags of the three raster passes: the light's cull view writes the list the ShadowMap pass draws.
The post exchange (UR_FRAME_POST_EXCHANGE) on these frames is not covered here: the helper of tests/test_gpu_post_band.py builds its
frames over an imported G-buffer with flags of its own."""
import numpy as np
import pytest

from tests.test_gbuffer_tex_ref import BAND_SPLITS, soup_reference

pytestmark = pytest.mark.gpu

W, H, SEED = 257, 130, 2
MAP = 64
BAND_NAMES = ("A", "B", "C", "hdr", "keys", "object_id")
WHOLE_NAMES = ("depth", "shadow", "hzb", "visible", "count", "args", "shadow_visible", "shadow_count", "gbuffer_stats", "depth_stats", "shadow_stats")


class _Shared:
    """What every frame of the test reads: the soup's draws and materials on the device, the constants with the soup's camera and a
    light that looks at the soup, the bounds, the lighting tables' sources."""

    def __init__(self, hp):
        from tests import gbuffer_tex_ref as X
        from tests.gbuffer_gpu import device_draws
        from tests.gbuffer_tex_gpu import device_materials
        from unclerenderer_amd import hostmath, synth
        from unclerenderer_amd.hotpath import HzbLayout, to_device
        self.hp = hp
        self.draws, self.view, self.proj, self.ref_depth, self.ref = soup_reference(W, H, SEED)
        self.mats = X.soup_materials(SEED)
        self.n = len(self.draws)
        self.dd = device_draws(self.draws)
        self.dm = device_materials(self.mats)
        self.args0 = to_device(self.dd.host_commands)
        self.shadow_commands = self.dd.commands  # the shadow pass's own slots: InstanceCount 1 whatever the camera's cull decides
        bounds = np.zeros((self.n, 2, 4), np.float32)
        every = []
        for k, d in enumerate(self.draws):
            p = np.ascontiguousarray(d.vertices).view(np.float32).reshape(-1, 16)[:, :3]
            bounds[k, 0, :3], bounds[k, 1, :3] = p.min(axis=0), p.max(axis=0)
            every.append(p)
        assert np.isfinite(bounds).all()
        self.bounds = to_device(bounds)
        self.fc = fc = hostmath.build_frame_constants("sponza", W, H, shadow_size=MAP, env_mip_count=5)
        fc.scene.View[:] = [float(v) for v in self.view]
        fc.scene.Projection[:] = [float(v) for v in self.proj]
        every = np.concatenate(every)
        centre = np.median(every, axis=0).astype(np.float32)
        self.lvp = hostmath.light_view_projection(centre, 4.0, fc.light_direction)
        fc.scene.LightViewProjection[:] = [float(v) for v in self.lvp]
        assert tuple(int(v) for v in fc.scene.ShadowMapSize) == (MAP, MAP)
        self.planes = hostmath.frustum_planes(self.lvp)
        self.consts = hostmath.pack_culling_constants(self.view, self.proj, 0, False, 0, 0, 0, True)
        self.env, self.lut = hp.stage_env_cube(synth.env_cube_procedural(16, 5), 16, 5), to_device(synth.brdf_lut_procedural(64, 16))
        self.lay = HzbLayout(W, H)
        self.hzb_valid = np.zeros(self.lay.total, bool)
        for off, mw, mh in self.lay.as_list():
            self.hzb_valid[off:off + mw * mh] = True


class _BandFrame:
    """A Frame over rows [row0, row0 + rows) with targets of its own: rows x W A, B, C, HDR, keys and ObjectId; whole-size depth, shadow
    map and HZB; depth_band the window depth[row0:row0 + rows] of the buffer the depth pass renders."""

    def __init__(self, sh: _Shared, row0: int, rows: int):
        import torch
        from unclerenderer_amd.hotpath import Frame, gbuffer_targets
        self.sh, self.row0, self.rows = sh, row0, rows
        half = lambda: torch.full((rows, W, 4), float("nan"), dtype=torch.float16, device="cuda")  # noqa: E731
        word = lambda: torch.full((rows, W), 0x5A5A5A5A, dtype=torch.int32, device="cuda")  # noqa: E731
        self.a, self.b, self.hdr, self.c, self.keys, self.oid = half(), half(), half(), word(), word(), word()
        self.depth = torch.full((H, W), 0.625, dtype=torch.float32, device="cuda")
        self.shadow = torch.full((MAP, MAP), 0.625, dtype=torch.float32, device="cuda")
        self.hzb = torch.full((sh.lay.total,), -1.0, device="cuda")
        self.args = sh.args0.clone()
        i32 = lambda n, v=-1: torch.full((n,), v, dtype=torch.int32, device="cuda")  # noqa: E731
        self.vis, self.cnt, self.svis, self.scnt = i32(sh.n), i32(1), i32(sh.n), i32(1)
        self.cull_stats, self.sstats, self.dstats, self.gstats = i32(2, 0), i32(4, 0), i32(6, 0), i32(6, 0)
        self.frame = Frame(sh.hp)
        self.frame.set_cull_views([dict(planes=sh.planes, visible_idx=self.svis, visible_count=self.scnt)])
        self.frame.set_shadow_pass(sh.shadow_commands, self.shadow, visible=(self.svis, self.scnt), stats=self.sstats)
        self.frame.set_depth_pass(self.args, self.depth, visible=(self.vis, self.cnt), stats=self.dstats)
        self.frame.set_gbuffer_pass(self.args, gbuffer_targets(self.a, self.b, self.c, self.hdr, self.keys, self.oid), visible=(self.vis, self.cnt), stats=self.gstats)
        self.frame.set_gbuffer_materials(sh.dm)

    def render(self, flags):
        from unclerenderer_amd.hotpath import Frame
        sh = self.sh
        self.args.copy_(sh.args0)
        for t in (self.sstats, self.dstats, self.gstats, self.cull_stats):
            t.zero_()
        self.tables = sh.hp.make_tables(self.shadow, sh.env, 16, 5, sh.lut)
        res = Frame.resources(W, H, self.row0, self.rows, self.a, self.b, self.c, self.depth[self.row0:self.row0 + self.rows], self.hdr, self.depth, self.hzb,
                              sh.lay, self.tables, sh.bounds, self.args, sh.n, 0, self.vis, self.cnt, self.cull_stats)
        self.frame.render(res, sh.consts, sh.fc.scene, sh.fc.sky, flags)

    def outputs(self):
        u16, u32 = (lambda t: t.cpu().numpy().view(np.uint16)), (lambda t: t.cpu().numpy().view(np.uint32))
        count, shadow_count = int(self.cnt.cpu()[0]), int(self.scnt.cpu()[0])
        hzb = u32(self.hzb)
        return {"A": u16(self.a), "B": u16(self.b), "hdr": u16(self.hdr), "C": u32(self.c), "keys": u32(self.keys), "object_id": u32(self.oid),
                "depth": u32(self.depth), "shadow": u32(self.shadow), "hzb": hzb[self.sh.hzb_valid], "visible": u32(self.vis)[:count], "count": np.uint32([count]),
                "args": u32(self.args), "shadow_visible": u32(self.svis)[:shadow_count], "shadow_count": np.uint32([shadow_count]),
                "gbuffer_stats": u32(self.gstats), "depth_stats": u32(self.dstats), "shadow_stats": u32(self.sstats)}

    def close(self):
        self.frame.close()


def _compare(whole, band, row0, rows, what, queued=False):
    """Every name that differs is reported. Of the GBuffer pass' stats6, [3] is compared only with a queue that holds every large
    triangle (it is then 0): it counts the large triangles that found no room, and whether a triangle is large is decided under the
    band's scissor; the other five count triangles whether or not they touch the band."""
    bad = [k for k in BAND_NAMES if not np.array_equal(band[k], whole[k][row0:row0 + rows])]
    bad += [k for k in WHOLE_NAMES if k != "gbuffer_stats" and not np.array_equal(band[k], whole[k])]
    counted = [0, 1, 2, 3, 4, 5] if queued else [0, 1, 2, 4, 5]
    if band["gbuffer_stats"][counted].tolist() != whole["gbuffer_stats"][counted].tolist():
        bad.append(f"gbuffer_stats {band['gbuffer_stats'].tolist()} against {whole['gbuffer_stats'].tolist()}")
    assert not bad, f"{what}: the frame over rows [{row0}, {row0 + rows}) differs from the whole frame in {bad}"


def _run_frames(frames, flags, count=2):
    import torch
    out = []
    for _ in range(count):  # the second frame culls against the first one's HZB
        for f in frames:
            f.render(flags)
        torch.cuda.synchronize()
        out.append([f.outputs() for f in frames])
    return out


@pytest.fixture(scope="module")
def shared(hotpath):
    return _Shared(hotpath)


@pytest.mark.parametrize("reserve", [1 << 16, 0])
@pytest.mark.parametrize("split", sorted(BAND_SPLITS))
def test_band_frames_equal_the_whole_frame(hotpath, shared, split, reserve):
    """Two frames each, on the main stream and with UR_FRAME_ASYNC_COMPUTE: every band's A, B, C, HDR, keys and ObjectId are the whole
    frame's rows; every band frame's depth, shadow map, HZB, lists, counts, InstanceCount words and stats are the whole frame's."""
    from unclerenderer_amd import lib
    flags = lib.UR_FRAME_DEFAULT | lib.UR_FRAME_CULL_VIEWS | lib.UR_FRAME_SHADOW_PASS | lib.UR_FRAME_DEPTH_PASS | lib.UR_FRAME_GBUFFER_PASS
    hotpath.raster_reserve(reserve)
    frames = []
    try:
        for lane in (0, lib.UR_FRAME_ASYNC_COMPUTE):
            frames = [_BandFrame(shared, 0, H)] + [_BandFrame(shared, r0, n) for r0, n in BAND_SPLITS[split]]
            for number, outs in enumerate(_run_frames(frames, flags | lane)):
                whole = outs[0]
                assert [r[0] for r in frames[0].frame.report()] == ["GPU Culling", "ShadowMap", "DepthPrepass", "GBuffer", "Build HZB", "Lighting", "Sky"]
                assert whole["count"][0] >= 1 and whole["shadow_count"][0] >= 1 and (whole["shadow"].view(np.float32) < 1).any()
                for f, o in zip(frames[1:], outs[1:]):
                    assert f.frame.report() == frames[0].frame.report()
                    _compare(whole, o, f.row0, f.rows, f"{split}, reserve {reserve}, lane {lane:#x}, frame {number}", queued=reserve != 0)
            for f in frames:
                f.close()
            frames = []
    finally:
        for f in frames:
            f.close()
        hotpath.raster_reserve(0)


def test_whole_frame_is_the_direct_calls_and_the_restatement(hotpath, shared):
    """The whole frame's depth is the restatement's, its G-buffer X.gbuffer_pass(..., select=order) under the cull's order, its HDR
    ur_deferred_lighting_sky by hand on ur_gbuffer_pass_materials' outputs: what the band frames are compared with is pinned."""
    import torch
    from tests import gbuffer_tex_ref as X
    from tests.gbuffer_gpu import same
    from unclerenderer_amd import lib
    from unclerenderer_amd.hotpath import gbuffer_targets
    sh = shared
    flags = lib.UR_FRAME_DEFAULT | lib.UR_FRAME_CULL_VIEWS | lib.UR_FRAME_SHADOW_PASS | lib.UR_FRAME_DEPTH_PASS | lib.UR_FRAME_GBUFFER_PASS
    f = _BandFrame(sh, 0, H)
    wanted = {}
    try:
        for number in range(2):
            got = _run_frames([f], flags, 1)[0][0]
            order = got["visible"].tolist()
            assert sorted(set(order)) == sorted(order) and len(order) >= 1
            if order == list(range(sh.n)):  # the cached reference's own selection
                wanted[tuple(order)] = (sh.ref_depth, sh.ref)
            if tuple(order) not in wanted:
                from tests import depth_ref as R
                depth, _ = R.depth_prepass(sh.draws, sh.view, sh.proj, W, H, slots=order)
                wanted[tuple(order)] = (depth, X.gbuffer_pass(sh.draws, sh.view, sh.proj, depth, W, H, materials=sh.mats, select=list(enumerate(order))))
            depth, want = wanted[tuple(order)]
            assert np.array_equal(got["depth"], depth.view(np.uint32)), number
            same({k: got[k] for k in ("A", "B", "C", "keys", "object_id")} | {"stats": got["gbuffer_stats"]}, want, f"the whole frame's G-buffer, frame {number}")
            a, b, hdr = (torch.zeros((H, W, 4), dtype=torch.float16, device="cuda") for _ in range(3))
            c, keys = (torch.zeros((H, W), dtype=torch.int32, device="cuda") for _ in range(2))
            hotpath.gbuffer_pass(sh.view, sh.proj, f.args, f.depth, gbuffer_targets(a, b, c, hdr, keys), W, H, visible=(f.vis, f.cnt), materials=sh.dm)
            assert np.array_equal(hdr.cpu().numpy().view(np.uint16), want["hdr"])
            hotpath.deferred_lighting_sky(sh.fc.scene, sh.fc.sky, a, b, c, f.depth, f.tables, hdr, W, H)
            torch.cuda.synchronize()
            assert np.array_equal(got["hdr"], hdr.cpu().numpy().view(np.uint16)), number
    finally:
        f.close()


def test_cleared_material_table_on_bands_gives_the_untextured_whole_frame(hotpath, shared):
    from unclerenderer_amd import lib
    flags = lib.UR_FRAME_DEFAULT | lib.UR_FRAME_CULL_VIEWS | lib.UR_FRAME_SHADOW_PASS | lib.UR_FRAME_DEPTH_PASS | lib.UR_FRAME_GBUFFER_PASS
    frames = [_BandFrame(shared, 0, H) for _ in range(2)] + [_BandFrame(shared, r0, n) for r0, n in BAND_SPLITS["2 x 65"]]
    try:
        for f in frames[1:]:
            f.frame.set_gbuffer_materials(None)
        for number, outs in enumerate(_run_frames(frames, flags)):
            textured, plain = outs[0], outs[1]
            assert not np.array_equal(plain["C"], textured["C"]) and np.array_equal(plain["keys"], textured["keys"])  # the maps were sampled
            for f, o in zip(frames[2:], outs[2:]):
                _compare(plain, o, f.row0, f.rows, f"no material table, frame {number}")
    finally:
        for f in frames:
            f.close()
