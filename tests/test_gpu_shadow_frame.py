"""The ShadowMap pass in the frame (UR_FRAME_SHADOW_PASS, ur_frame_set_shadow_pass) on small frames: 64 x 32 pixels, a 64 x 64 map.
The pass sits directly behind "GPU Culling", draws the list the light's cull view wrote in that pass, and Lighting samples its map."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, MAP = 64, 32, 64


def _quad(lvp, x0, x1, y0, y1, z):
    """Two triangles, clockwise on the light's target (back faces: drawn), at light clip depth z - as world positions."""
    inv = np.linalg.inv(np.asarray(lvp, np.float64).reshape(4, 4))
    clip = np.array([(x0, y1), (x1, y1), (x0, y0), (x1, y1), (x1, y0), (x0, y0)], np.float64)
    p = np.concatenate([clip, np.full((6, 1), z), np.ones((6, 1))], axis=1) @ inv
    return (p[:, :3] / p[:, 3:]).astype(np.float32)


class _Scene:
    def __init__(self, hotpath, models):
        """models: [(world positions (k, 3), AABB or None for the positions' own)]"""
        import torch
        from tests import shadow_ref as R
        from tests.shadow_gpu import DeviceDraws
        from unclerenderer_amd import hostmath, synth
        from unclerenderer_amd.hotpath import HzbLayout, to_device
        self.hp = hotpath
        self.fc = fc = hostmath.build_frame_constants("sponza", W, H, shadow_size=MAP, env_mip_count=5)
        self.lvp = np.array(list(fc.scene.LightViewProjection), np.float32)
        assert tuple(int(v) for v in fc.scene.ShadowMapSize) == (MAP, MAP)
        g = synth.gbuffer_scene(fc.view, fc.proj, fc.camera_position, W, H, 5)
        self.g = g
        self.env, self.lut = hotpath.stage_env_cube(synth.env_cube_procedural(16, 5), 16, 5), to_device(synth.brdf_lut_procedural(64, 16))
        self.lay = HzbLayout(W, H)
        self.dev = [to_device(a) for a in (g.A, g.B, g.C, g.depth)]
        self.hzb = torch.zeros(self.lay.total, device="cuda")
        self.consts = hostmath.pack_culling_constants(fc.view, fc.proj, 0, False, 0, 0, 0, True)
        models = [(np.asarray(p, np.float32), b) for p, b in models(self.lvp)]
        self.n = n = len(models)
        self.draws = [R.Draw(R.vertex_buffer(p), np.arange(p.shape[0], dtype=np.uint32)) for p, _ in models]
        self.dd = DeviceDraws(self.draws)  # the shadow pass's own commands: InstanceCount 1, whatever the camera's cull decides
        bounds = np.zeros((n, 2, 4), np.float32)
        for k, (p, b) in enumerate(models):
            bounds[k, 0, :3], bounds[k, 1, :3] = (p.min(axis=0) - 0.01, p.max(axis=0) + 0.01) if b is None else b
        self.bounds = to_device(bounds)
        self.args0 = synth.indirect_args_initial(n)
        self.args = to_device(self.args0)
        self.vis, self.cnt = torch.full((n,), -1, dtype=torch.int32, device="cuda"), torch.full((1,), -1, dtype=torch.int32, device="cuda")
        self.view = dict(planes=hostmath.frustum_planes(self.lvp), visible_idx=self.vis, visible_count=self.cnt)

    def tables(self, shadow):
        return self.hp.make_tables(shadow, self.env, 16, 5, self.lut)

    def render(self, frame, shadow, flags):
        import torch
        from unclerenderer_amd.hotpath import Frame, to_device
        hdr = to_device(self.g.hdr)
        self.args.copy_(to_device(self.args0))
        a, b, c, d = self.dev
        res = Frame.resources(W, H, 0, H, a, b, c, d, hdr, d, self.hzb, self.lay, self.tables(shadow), self.bounds, self.args, self.n, 0, None, None, None)
        frame.reset_hzb()
        frame.render(res, self.consts, self.fc.scene, self.fc.sky, flags)
        torch.cuda.synchronize()
        return hdr.cpu().numpy()


def _two_models(lvp):
    occluder = _quad(lvp, -1.0, 1.0, -1.0, 1.0, 0.05)  # covers the whole map, close to the light
    liar = _quad(lvp, -0.5, 0.5, -0.5, 0.5, 0.02)      # would darken the middle of the map - but its AABB lies far outside the light's frustum
    far = _quad(lvp, 40.0, 41.0, 40.0, 41.0, 0.5)
    return [(occluder, None), (liar, (far.min(axis=0), far.max(axis=0)))]


def test_shadow_pass_in_the_frame(hotpath):
    import torch
    from tests import shadow_ref as R
    from unclerenderer_amd import lib
    from unclerenderer_amd.hotpath import Frame
    s = _Scene(hotpath, _two_models)
    flags = lib.UR_FRAME_DEFAULT | lib.UR_FRAME_CULL_VIEWS
    sentinel = 0.625
    shadow = torch.full((MAP, MAP), sentinel, dtype=torch.float32, device="cuda")
    stats = torch.zeros(4, dtype=torch.int32, device="cuda")
    frame = Frame(hotpath)
    frame.set_cull_views([s.view])
    frame.set_shadow_pass(s.dd.commands, shadow, visible=(s.vis, s.cnt), stats=stats)

    # ---- without the flag: today's frame, and the pass's map is not touched
    hdr_plain = s.render(frame, shadow, flags)
    rep_plain = frame.report()
    assert [r[0] for r in rep_plain] == ["GPU Culling", "Build HZB", "Lighting", "Sky"]
    assert (shadow.cpu().numpy() == np.float32(sentinel)).all() and not stats.cpu().numpy().any()
    bare = Frame(hotpath)
    bare.set_cull_views([s.view])
    assert np.array_equal(s.render(bare, shadow, flags), hdr_plain) and bare.report() == rep_plain

    # ---- with the flag: ShadowMap directly behind GPU Culling, drawing the light view's list
    hdr = s.render(frame, shadow, flags | lib.UR_FRAME_SHADOW_PASS)
    rep = frame.report()
    assert [r[0] for r in rep] == ["GPU Culling", "ShadowMap", "Build HZB", "Lighting", "Sky"] and not any(r[1] for r in rep)
    assert int(s.cnt.cpu()[0]) == 1 and int(s.vis.cpu()[0]) == 0, "the light view accepts the occluder and rejects the model whose bounds lie outside"
    got = shadow.cpu().numpy()
    want, want_stats = R.shadow_map(s.draws, s.lvp, MAP, MAP, slots=[0])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert stats.cpu().numpy()[:3].tolist() == want_stats.tolist() == [2, 0, 0]
    assert (got < 1).all(), "the occluder covers the whole map"
    with_liar, _ = R.shadow_map(s.draws, s.lvp, MAP, MAP)
    assert not np.array_equal(with_liar, want), "the rejected model would have changed the map"

    # ---- the same bytes as ur_shadow_map followed by a frame without the flag on that map
    alone = torch.zeros((MAP, MAP), dtype=torch.float32, device="cuda")
    hotpath.shadow_map(s.lvp, s.dd.commands, alone, visible=(s.vis, s.cnt))
    torch.cuda.synchronize()
    assert torch.equal(alone, shadow)
    assert np.array_equal(s.render(bare, alone, flags), hdr)

    # ---- the accepted occluder darkens what lies under it: against a map nothing was drawn into
    lit = s.render(bare, torch.ones((MAP, MAP), dtype=torch.float32, device="cuda"), flags)
    a, b = hdr.view(np.float16).astype(np.float32)[..., :3], lit.view(np.float16).astype(np.float32)[..., :3]
    assert (a <= b).all() and (a < b).any()

    # ---- shadows off: the pass is listed and culled, as in the reference, and the map stays
    shadow.fill_(sentinel)
    s.render(frame, shadow, (flags | lib.UR_FRAME_SHADOW_PASS) & ~lib.UR_FRAME_SHADOWS)
    assert ("ShadowMap", True, 0) in frame.report() and (shadow.cpu().numpy() == np.float32(sentinel)).all()

    # ---- async compute: the cull runs on the second stream, the pass on the main one behind a wait on it
    shadow.fill_(sentinel)
    hdr_async = s.render(frame, shadow, flags | lib.UR_FRAME_SHADOW_PASS | lib.UR_FRAME_ASYNC_COMPUTE)
    lanes = {n: (a, w) for n, a, w in frame.report_async()}
    assert lanes["GPU Culling"][0] and not lanes["ShadowMap"][0] and lanes["ShadowMap"][1] >= 1
    assert np.array_equal(shadow.cpu().numpy().view(np.uint32), want.view(np.uint32)) and np.array_equal(hdr_async, hdr)

    # ---- Lighting must read the map the pass renders
    other = torch.ones((MAP, MAP), dtype=torch.float32, device="cuda")
    with pytest.raises(lib.UrError) as e:
        s.render(frame, other, flags | lib.UR_FRAME_SHADOW_PASS)
    assert e.value.code == lib.UR_EINVAL
    frame.close(); bare.close()


def test_rejected_occluder_alone_leaves_the_map_clear(hotpath):
    import torch
    from unclerenderer_amd import lib
    from unclerenderer_amd.hotpath import Frame
    s = _Scene(hotpath, lambda lvp: _two_models(lvp)[1:])
    shadow = torch.zeros((MAP, MAP), dtype=torch.float32, device="cuda")
    stats = torch.zeros(4, dtype=torch.int32, device="cuda")
    frame = Frame(hotpath)
    frame.set_cull_views([s.view])
    frame.set_shadow_pass(s.dd.commands, shadow, visible=(s.vis, s.cnt), stats=stats)
    s.render(frame, shadow, lib.UR_FRAME_DEFAULT | lib.UR_FRAME_CULL_VIEWS | lib.UR_FRAME_SHADOW_PASS)
    assert int(s.cnt.cpu()[0]) == 0
    assert (shadow.cpu().numpy() == 1.0).all() and not stats.cpu().numpy().any()
    frame.close()
