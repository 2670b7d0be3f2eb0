"""The textured GBuffer pass in the frame (ur_frame_set_gbuffer_materials) on a 64 x 64 frame: two frames of cull -> DepthPrepass -> GBuffer
-> Lighting -> Sky with a material table set are byte-equal to the direct calls (ur_gbuffer_pass_materials, then
ur_deferred_lighting_sky) and to the restatement; clearing the table gives back the untextured frame's bytes."""
import numpy as np
import pytest

from tests.test_gpu_gbuffer_frame import H, W, _Scene

pytestmark = pytest.mark.gpu


def _textured_scene(hotpath):
    """tests/test_gpu_gbuffer_frame.py's scene with seeded TEXCOORDs and tangents in its vertices."""
    from tests.gbuffer_gpu import device_draws
    from unclerenderer_amd.hotpath import to_device
    s = _Scene(hotpath)
    rng = np.random.default_rng(9)
    for d in s.draws:
        v = d.vertices.view(np.float32).reshape(-1, 16)
        v[:, 6:8] = rng.uniform(-3, 3, (v.shape[0], 2))
        v[:, 8:11] = rng.normal(size=(v.shape[0], 3))
        v[:, 11] = 1.0
    s.dd = device_draws(s.draws)
    s.args0 = s.dd.host_commands.copy()
    s.args = to_device(s.args0)
    return s


def test_two_frames_with_materials_and_cleared(hotpath):
    import torch
    from tests import depth_ref as R
    from tests import gbuffer_tex_ref as X
    from tests.gbuffer_gpu import same
    from tests.gbuffer_tex_gpu import device_materials
    from unclerenderer_amd import lib
    from unclerenderer_amd.hotpath import Frame, gbuffer_targets
    s = _textured_scene(hotpath)
    rng = np.random.default_rng(4)
    mats = [{"key": 15 - 2 * k, **{name: X.random_texture(*X.TEXTURE_SHAPES[(k + j) % 2], name == "base_color", rng) for j, (name, _, _) in enumerate(X.MAPS)}}
            for k in range(s.n)]
    dm = device_materials(mats)
    flags = lib.UR_FRAME_DEFAULT | lib.UR_FRAME_DEPTH_PASS | lib.UR_FRAME_GBUFFER_PASS
    frame = Frame(hotpath)
    s.set_passes(frame)
    s.render(frame, flags)
    plain = s.outputs()
    s.render(frame, flags)
    plain_report = frame.report()  # of a frame with a frame in front of it, as the textured ones below (the first frame's transitions differ)
    assert [r[0] for r in plain_report] == ["GPU Culling", "DepthPrepass", "GBuffer", "Build HZB", "Lighting", "Sky"]
    frame.set_gbuffer_materials(dm)
    depth, _ = R.depth_prepass(s.draws, s.view, s.proj, W, H)
    for _ in range(2):  # the second frame culls against the first one's HZB
        s.gstats.zero_()
        tables = s.render(frame, flags)
        assert frame.report() == plain_report
        order = s.vis.cpu().numpy()[:int(s.cnt.cpu()[0])].tolist()
        want = X.gbuffer_pass(s.draws, s.view, s.proj, depth, W, H, materials=mats, select=list(enumerate(order)))
        got = {"A": s.a.cpu().numpy().view(np.uint16), "B": s.b.cpu().numpy().view(np.uint16), "C": s.c.cpu().numpy().view(np.uint32),
               "keys": s.keys.cpu().numpy().view(np.uint32), "object_id": s.oid.cpu().numpy().view(np.uint32), "stats": s.gstats.cpu().numpy().view(np.uint32)}
        same(got, want, "the frame's textured G-buffer")
        assert set(want["shade32"]["bits"].tolist()) == {15, 13}
        a, b, hdr = (torch.zeros((H, W, 4), dtype=torch.float16, device="cuda") for _ in range(3))
        c, keys = (torch.zeros((H, W), dtype=torch.int32, device="cuda") for _ in range(2))
        hotpath.gbuffer_pass(s.view, s.proj, s.args, s.depth, gbuffer_targets(a, b, c, hdr, keys), W, H, visible=(s.vis, s.cnt), materials=dm)
        assert np.array_equal(hdr.cpu().numpy().view(np.uint16), want["hdr"])
        hotpath.deferred_lighting_sky(s.fc.scene, s.fc.sky, a, b, c, s.depth, tables, hdr, W, H)
        torch.cuda.synchronize()
        assert np.array_equal(s.hdr.cpu().numpy().view(np.uint16), hdr.cpu().numpy().view(np.uint16))
    textured = s.outputs()
    assert not np.array_equal(textured[2], plain[2])  # gbuffer_c differs: the maps were sampled
    # clearing the table: the untextured frame's bytes (a fresh frame for the same HZB history as `plain`)
    frame.set_gbuffer_materials(None)
    frame.reset_hzb()
    s.render(frame, flags)
    for x, y in zip(plain, s.outputs()):
        assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8))
    frame.close()
