"""The GBuffer pass in the frame (UR_FRAME_GBUFFER_PASS, ur_frame_set_gbuffer_pass) on a 64 x 64 frame: cull -> DepthPrepass -> GBuffer ->
Lighting -> Sky with no imported G-buffer: the HDR band is byte-equal to ur_deferred_lighting_sky called by hand on ur_gbuffer_pass'
outputs; without the flag nothing changes."""
import numpy as np
import pytest

from tests.test_gpu_depth_frame import _quad

pytestmark = pytest.mark.gpu

W, H = 64, 64


class _Scene:
    def __init__(self, hotpath):
        import torch
        from tests import gbuffer_ref as G
        from tests.gbuffer_gpu import device_draws
        from unclerenderer_amd import hostmath, synth
        from unclerenderer_amd.hotpath import HzbLayout, gbuffer_targets, to_device
        self.hp = hotpath
        self.fc = fc = hostmath.build_frame_constants("sponza", W, H, shadow_size=64, env_mip_count=5)
        self.view, self.proj = np.array(list(fc.scene.View), np.float32), np.array(list(fc.scene.Projection), np.float32)
        self.g = synth.gbuffer_scene(fc.view, fc.proj, fc.camera_position, W, H, 5)
        self.env, self.lut = hotpath.stage_env_cube(synth.env_cube_procedural(16, 5), 16, 5), to_device(synth.brdf_lut_procedural(64, 16))
        self.shadow = torch.ones((64, 64), dtype=torch.float32, device="cuda")
        self.lay = HzbLayout(W, H)
        models = [_quad(self.view, self.proj, -0.8, 0.6, -0.7, 0.9, 5.0), _quad(self.view, self.proj, -0.2, 0.95, -0.9, 0.2, 3.0)]
        rng = np.random.default_rng(3)
        self.n = len(models)
        self.draws = [G.GDraw(G.vertex_buffer(p, normals=rng.normal(size=(6, 3)) + [0, 0, -3], colors=rng.uniform(0, 1, (6, 3))), np.arange(6, dtype=np.uint32),
                              base_color=rng.uniform(0.2, 1, 3).astype(np.float32), emissive=rng.uniform(0, 0.5, 3).astype(np.float32),
                              metallic=0.25 * k, roughness=0.5 + 0.25 * k, object_id=100 + k) for k, p in enumerate(models)]
        self.dd = device_draws(self.draws)
        self.args0 = self.dd.host_commands.copy()
        bounds = np.zeros((self.n, 2, 4), np.float32)
        for k, p in enumerate(models):
            bounds[k, 0, :3], bounds[k, 1, :3] = p.min(axis=0) - 0.01, p.max(axis=0) + 0.01
        self.bounds = to_device(bounds)
        self.consts = hostmath.pack_culling_constants(fc.view, fc.proj, 0, False, 0, 0, 0, True)
        self.args = to_device(self.args0)
        self.vis = torch.full((self.n,), -1, dtype=torch.int32, device="cuda")
        self.cnt = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        self.cull_stats = torch.zeros(2, dtype=torch.int32, device="cuda")
        self.hzb = torch.full((self.lay.total,), -1.0, device="cuda")
        self.depth = torch.full((H, W), 0.625, dtype=torch.float32, device="cuda")
        self.a, self.b, self.hdr = (torch.zeros((H, W, 4), dtype=torch.float16, device="cuda") for _ in range(3))
        self.c, self.keys, self.oid = (torch.zeros((H, W), dtype=torch.int32, device="cuda") for _ in range(3))
        self.targets = gbuffer_targets(self.a, self.b, self.c, self.hdr, self.keys, self.oid)
        self.dstats, self.gstats = (torch.zeros(6, dtype=torch.int32, device="cuda") for _ in range(2))

    def imported(self):
        from unclerenderer_amd.hotpath import to_device
        for t, a in ((self.a, self.g.A), (self.b, self.g.B), (self.c, self.g.C), (self.hdr, self.g.hdr)):
            t.copy_(to_device(a).view(t.dtype).reshape(t.shape))

    def set_passes(self, frame, **kw):
        frame.set_depth_pass(self.args, self.depth, visible=(self.vis, self.cnt), stats=self.dstats)
        frame.set_gbuffer_pass(self.args, kw.pop("targets", self.targets), visible=(self.vis, self.cnt), stats=self.gstats, **kw)

    def render(self, frame, flags, depth_band=None):
        import torch
        from unclerenderer_amd.hotpath import Frame, to_device
        self.args.copy_(to_device(self.args0))
        tables = self.hp.make_tables(self.shadow, self.env, 16, 5, self.lut)
        res = Frame.resources(W, H, 0, H, self.a, self.b, self.c, self.depth if depth_band is None else depth_band, self.hdr, self.depth, self.hzb, self.lay,
                              tables, self.bounds, self.args, self.n, 0, self.vis, self.cnt, self.cull_stats)
        frame.render(res, self.consts, self.fc.scene, self.fc.sky, flags)
        torch.cuda.synchronize()
        return tables

    def outputs(self):
        return [t.cpu().numpy().copy() for t in (self.a, self.b, self.c, self.hdr, self.depth, self.hzb, self.args, self.cnt, self.cull_stats)]


def test_frame_from_geometry_to_hdr(hotpath):
    import torch
    from tests import depth_ref as R
    from tests import gbuffer_ref as G
    from tests.gbuffer_gpu import same
    from unclerenderer_amd import lib
    from unclerenderer_amd.hotpath import Frame, gbuffer_targets
    s = _Scene(hotpath)
    flags = lib.UR_FRAME_DEFAULT | lib.UR_FRAME_DEPTH_PASS | lib.UR_FRAME_GBUFFER_PASS
    frame = Frame(hotpath)
    s.set_passes(frame)
    tables = s.render(frame, flags)
    rep = frame.report()
    assert [r[0] for r in rep] == ["GPU Culling", "DepthPrepass", "GBuffer", "Build HZB", "Lighting", "Sky"] and not any(r[1] for r in rep)
    # the G-buffer is the restatement's, against the depth the prepass rendered
    depth, _ = R.depth_prepass(s.draws, s.view, s.proj, W, H)
    assert np.array_equal(s.depth.cpu().numpy().view(np.uint32), depth.view(np.uint32))
    order = s.vis.cpu().numpy()[:int(s.cnt.cpu()[0])].tolist()
    assert sorted(order) == [0, 1]
    want = G.gbuffer_pass(s.draws, s.view, s.proj, depth, W, H, select=list(enumerate(order)))
    got = {"A": s.a.cpu().numpy().view(np.uint16), "B": s.b.cpu().numpy().view(np.uint16), "C": s.c.cpu().numpy().view(np.uint32),
           "keys": s.keys.cpu().numpy().view(np.uint32), "object_id": s.oid.cpu().numpy().view(np.uint32), "stats": s.gstats.cpu().numpy().view(np.uint32)}
    same(got, want, "the frame's G-buffer")
    assert (want["keys"] != 0).mean() > 0.3 and (want["keys"] == 0).any()
    # the HDR band: ur_deferred_lighting_sky by hand on ur_gbuffer_pass' outputs
    a, b, hdr = (torch.zeros((H, W, 4), dtype=torch.float16, device="cuda") for _ in range(3))
    c, keys = (torch.zeros((H, W), dtype=torch.int32, device="cuda") for _ in range(2))
    hotpath.gbuffer_pass(s.view, s.proj, s.args, s.depth, gbuffer_targets(a, b, c, hdr, keys), W, H, visible=(s.vis, s.cnt))
    assert np.array_equal(hdr.cpu().numpy().view(np.uint16), want["hdr"])
    hotpath.deferred_lighting_sky(s.fc.scene, s.fc.sky, a, b, c, s.depth, tables, hdr, W, H)
    torch.cuda.synchronize()
    assert np.array_equal(s.hdr.cpu().numpy().view(np.uint16), hdr.cpu().numpy().view(np.uint16))
    first = s.outputs()
    # the async-compute lane: the same bytes, the pass on the main stream
    other = Frame(hotpath)
    s.set_passes(other)
    other.reset_hzb()
    frame.reset_hzb()
    s.render(frame, flags)
    ref = s.outputs()
    s.render(other, flags | lib.UR_FRAME_ASYNC_COMPUTE)
    for x, y in zip(ref, s.outputs()):
        assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8))
    lanes = {n: (a_, w_) for n, a_, w_ in other.report_async()}
    assert lanes["GPU Culling"][0] and not lanes["GBuffer"][0], lanes
    other.close()
    del first

    # ---- the UR_EINVAL cases of the flag
    def refused(text, fl=flags, **kw):
        s.set_passes(frame, **kw)
        with pytest.raises(lib.UrError) as e:
            s.render(frame, fl)
        assert e.value.code == lib.UR_EINVAL and text in str(e.value), str(e.value)

    refused("UR_FRAME_DEPTH_PASS", flags & ~lib.UR_FRAME_DEPTH_PASS)
    refused("quantise", flags=lib.UR_DEPTH_QUANTIZE_D24)
    spare = torch.zeros((H, W, 4), dtype=torch.float16, device="cuda")
    refused("same buffers", targets=gbuffer_targets(spare, s.b, s.c, s.hdr, s.keys))
    refused("same buffers", targets=gbuffer_targets(s.a, s.b, s.c, spare, s.keys))
    frame.set_gbuffer_pass()
    with pytest.raises(lib.UrError) as e:
        s.render(frame, flags)
    assert e.value.code == lib.UR_EINVAL and "ur_frame_set_gbuffer_pass" in str(e.value)
    frame.close()


def test_without_the_flag_nothing_changes(hotpath):
    """The report and every output of a frame over an imported G-buffer are byte-equal before and after the pass struct is set. Sky
    reads the imported G-buffer's own depth, as with every imported G-buffer: where that G-buffer holds no surface its normal is zero,
    Lighting leaves a NaN and Sky overwrites it. Bytes are compared, so a NaN that stayed would still have to be the same NaN."""
    from unclerenderer_amd import lib
    from unclerenderer_amd.hotpath import Frame, to_device
    s = _Scene(hotpath)
    band = to_device(s.g.depth)
    flags = lib.UR_FRAME_DEFAULT | lib.UR_FRAME_DEPTH_PASS
    bare = Frame(hotpath)
    bare.set_depth_pass(s.args, s.depth, visible=(s.vis, s.cnt), stats=s.dstats)
    s.imported()
    s.render(bare, flags, depth_band=band)
    before, rep_before = s.outputs(), bare.report()
    assert [r[0] for r in rep_before] == ["GPU Culling", "DepthPrepass", "Build HZB", "Lighting", "Sky"]
    frame = Frame(hotpath)
    s.set_passes(frame)
    s.imported()
    s.render(frame, flags, depth_band=band)
    assert frame.report() == rep_before
    for x, y in zip(before, s.outputs()):
        assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8))
    assert not s.gstats.cpu().numpy().any() and not s.keys.cpu().numpy().any()
    bare.close(); frame.close()
