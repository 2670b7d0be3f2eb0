"""The DepthPrepass pass in the frame (UR_FRAME_DEPTH_PASS, ur_frame_set_depth_pass) on a 64 x 32 frame: cull -> DepthPrepass ->
Build HZB -> the next frame's cull, with no imported depth. A wall covers the screen and an instance stands behind it: frame 1 culls
without an HZB and draws both, frame 2's cull drops the hidden one against the HZB of the depth frame 1 rendered."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 64, 32


def _quad(view, proj, x0, x1, y0, y1, z):
    """Two triangles, counter-clockwise on the target (front faces: drawn), over NDC [x0, x1] x [y0, y1] at view depth z - world positions."""
    xs, ys = float(proj[0]), float(proj[5])
    ndc = np.array([(x0, y1), (x0, y0), (x1, y1), (x1, y1), (x0, y0), (x1, y0)], np.float64)
    pv = np.concatenate([ndc[:, :1] * z / xs, ndc[:, 1:] * z / ys, np.full((6, 1), z), np.ones((6, 1))], axis=1)
    return (pv @ np.linalg.inv(np.asarray(view, np.float64).reshape(4, 4)))[:, :3].astype(np.float32)


class _Scene:
    def __init__(self, hotpath):
        import torch
        from tests import depth_ref as R
        from tests.shadow_gpu import DeviceDraws
        from unclerenderer_amd import hostmath, synth
        from unclerenderer_amd.hotpath import HzbLayout, to_device
        self.hp = hotpath
        self.fc = fc = hostmath.build_frame_constants("sponza", W, H, shadow_size=64, env_mip_count=5)
        self.view, self.proj = np.array(list(fc.scene.View), np.float32), np.array(list(fc.scene.Projection), np.float32)
        g = synth.gbuffer_scene(fc.view, fc.proj, fc.camera_position, W, H, 5)
        self.g = g
        self.env, self.lut = hotpath.stage_env_cube(synth.env_cube_procedural(16, 5), 16, 5), to_device(synth.brdf_lut_procedural(64, 16))
        self.shadow = torch.ones((64, 64), dtype=torch.float32, device="cuda")
        self.lay = HzbLayout(W, H)
        self.gbuf = [to_device(a) for a in (g.A, g.B, g.C)]
        self.depth_band = to_device(g.depth)  # Sky's input: the G-buffer's depth, not the prepass's
        models = [_quad(self.view, self.proj, -1.3, 1.3, -1.3, 1.3, 5.0), _quad(self.view, self.proj, -0.2, 0.2, -0.2, 0.2, 10.0)]
        self.n = len(models)
        self.draws = [R.Draw(R.vertex_buffer(p), np.arange(6, dtype=np.uint32)) for p in models]
        self.dd = DeviceDraws(self.draws)
        self.args0 = self.dd.host_commands.copy()  # the cull's own slots: it writes their InstanceCount, the prepass draws them
        bounds = np.zeros((self.n, 2, 4), np.float32)
        for k, p in enumerate(models):
            bounds[k, 0, :3], bounds[k, 1, :3] = p.min(axis=0) - 0.01, p.max(axis=0) + 0.01
        self.host_bounds = bounds
        self.bounds = to_device(bounds)
        self.consts = hostmath.pack_culling_constants(fc.view, fc.proj, 0, False, 0, 0, 0, True)
        self.fresh()

    def fresh(self):
        import torch
        from unclerenderer_amd.hotpath import to_device
        self.args = to_device(self.args0)
        self.vis = torch.full((self.n,), -1, dtype=torch.int32, device="cuda")
        self.cnt = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        self.cull_stats = torch.zeros(2, dtype=torch.int32, device="cuda")
        self.hzb = torch.full((self.lay.total,), -1.0, device="cuda")
        self.depth = torch.full((H, W), 0.625, dtype=torch.float32, device="cuda")
        self.stats = torch.zeros(6, dtype=torch.int32, device="cuda")
        self.hdr = torch.zeros((H, W, 4), dtype=torch.float16, device="cuda")

    def set_pass(self, frame):
        frame.set_depth_pass(self.args, self.depth, visible=(self.vis, self.cnt), stats=self.stats)

    def render(self, frame, flags, depth_full=None):
        import torch
        from unclerenderer_amd.hotpath import Frame, to_device
        self.args.copy_(to_device(self.args0))
        self.hdr.copy_(to_device(self.g.hdr))
        a, b, c = self.gbuf
        tables = self.hp.make_tables(self.shadow, self.env, 16, 5, self.lut)
        res = Frame.resources(W, H, 0, H, a, b, c, self.depth_band, self.hdr, self.depth if depth_full is None else depth_full, self.hzb, self.lay, tables,
                              self.bounds, self.args, self.n, 0, self.vis, self.cnt, self.cull_stats)
        frame.render(res, self.consts, self.fc.scene, self.fc.sky, flags)
        torch.cuda.synchronize()

    def outputs(self):
        return [t.cpu().numpy().copy() for t in (self.depth, self.hzb, self.args, self.vis, self.cnt, self.cull_stats, self.stats, self.hdr)]


def _two_frames(s, frame, flags):
    """Frame 1 without an HZB, frame 2 against frame 1's: the outputs after each."""
    frame.reset_hzb()
    s.render(frame, flags)
    first = s.outputs()
    s.stats.zero_(); s.cull_stats.zero_()
    s.render(frame, flags)
    return first, s.outputs()


def test_closed_visibility_loop(hotpath):
    import torch
    from tests import depth_ref as R
    from tests import visibility_ref as V
    from unclerenderer_amd import lib
    from unclerenderer_amd.hotpath import Frame
    s = _Scene(hotpath)
    flags = lib.UR_FRAME_DEFAULT | lib.UR_FRAME_DEPTH_PASS
    frame = Frame(hotpath)
    s.set_pass(frame)
    first, second = _two_frames(s, frame, flags)
    rep = frame.report()
    assert [r[0] for r in rep] == ["GPU Culling", "DepthPrepass", "Build HZB", "Lighting", "Sky"] and not any(r[1] for r in rep)

    # ---- frame 1: no HZB yet, both instances pass the frustum and are drawn; the depth is the restatement's, the HZB is built from it
    depth1, hzb1, args1, vis1, cnt1, _, stats1, hdr1 = first
    assert int(cnt1[0]) == 2 and sorted(vis1.tolist()) == [0, 1] and args1.view(np.uint32).reshape(-1, 16)[:, 11].tolist() == [1, 1]
    want, want_stats = R.depth_prepass(s.draws, s.view, s.proj, W, H)
    assert np.array_equal(depth1.view(np.uint32), want.view(np.uint32))
    assert stats1.view(np.uint32)[[0, 1, 2, 4, 5]].tolist() == want_stats[[0, 1, 2, 4, 5]].tolist() == [4, 0, 0, 0, 0]
    assert (want > 0).all(), "the wall covers the screen"
    alone = torch.full((s.lay.total,), -1.0, device="cuda")
    hotpath.build_hzb(torch.from_numpy(want.copy()).to("cuda"), alone, s.lay)
    torch.cuda.synchronize()
    assert np.array_equal(hzb1.view(np.uint32), alone.cpu().numpy().view(np.uint32))

    # ---- frame 2: the cull reads that HZB and drops the instance behind the wall, as the restatement of the cull decides
    depth2, hzb2, args2, vis2, cnt2, cull2, stats2, hdr2 = second
    c = np.array(s.consts, np.uint32)
    c[40], c[41], c[42], c[43], c[44] = s.n, 1, s.lay.count, s.lay.width, s.lay.height
    exp_args, exp_stats, exp_list, exp_count = V.expected_outputs(c, s.host_bounds, hzb1, s.lay.as_list(), s.args0)
    assert exp_count == 1 and list(exp_list) == [0], "the restatement keeps the wall and drops the hidden instance"
    assert np.array_equal(args2.view(np.uint32).reshape(-1, 16), exp_args) and int(cnt2[0]) == exp_count and vis2[:exp_count].tolist() == list(exp_list)
    assert np.array_equal(cull2.view(np.uint32), exp_stats) and exp_stats[1] == 1
    # its prepass draws the camera's list - the wall alone - and the depth bytes are those of frame 1
    assert stats2.view(np.uint32)[0] == 2
    assert np.array_equal(depth2.view(np.uint32), depth1.view(np.uint32)) and np.array_equal(hzb2.view(np.uint32), hzb1.view(np.uint32))
    assert np.array_equal(hdr2, hdr1)

    # ---- the async-compute lane and both riding HZB chains: the same bytes, frame by frame
    for extra in (lib.UR_FRAME_ASYNC_COMPUTE, lib.UR_FRAME_HZB_WITH_LIGHTING, lib.UR_FRAME_HZB_TAIL_WITH_LIGHTING):
        s.fresh()
        other = Frame(hotpath)
        s.set_pass(other)
        f1, f2 = _two_frames(s, other, flags | extra)
        for got, ref, what in ((f1, first, "frame 1"), (f2, second, "frame 2")):
            for k, name in enumerate(("depth", "hzb", "args", "visible_idx", "visible_count", "cull_stats", "stats6", "lighting")):
                if name == "visible_idx":
                    n = int(ref[4][0])
                    assert sorted(got[k][:n].tolist()) == sorted(ref[k][:n].tolist()), (hex(extra), what, name)
                else:
                    assert np.array_equal(got[k], ref[k]), (hex(extra), what, name)
        if extra == lib.UR_FRAME_ASYNC_COMPUTE:
            lanes = {n: (a, w) for n, a, w in other.report_async()}
            assert lanes["GPU Culling"][0] and not lanes["DepthPrepass"][0] and lanes["DepthPrepass"][1] >= 1, lanes  # the wait on the cull
            assert lanes["Build HZB"][0] and lanes["Build HZB"][1] >= 1, lanes                                          # the wait on the prepass
        other.close()

    # ---- the prepass off: the pass is listed and culled, as in the reference, and the buffer stays
    s.set_pass(frame)  # (fresh() above replaced the buffers the first frame's pass pointed at)
    s.depth.fill_(0.625)
    s.render(frame, flags & ~lib.UR_FRAME_DEPTH_PREPASS)
    assert ("DepthPrepass", True, 0) in frame.report() and (s.depth.cpu().numpy() == np.float32(0.625)).all()

    # ---- Build HZB must read the buffer the pass renders
    with pytest.raises(lib.UrError) as e:
        s.render(frame, flags, depth_full=torch.zeros((H, W), dtype=torch.float32, device="cuda"))
    assert e.value.code == lib.UR_EINVAL
    frame.close()


def test_without_the_flag_nothing_changes(hotpath):
    """The report and every output of a frame are byte-equal before and after the pass struct is set; the pass's depth is only read."""
    from unclerenderer_amd import lib
    from unclerenderer_amd.hotpath import Frame
    s = _Scene(hotpath)
    flags = lib.UR_FRAME_DEFAULT
    bare = Frame(hotpath)
    before = _two_frames(s, bare, flags)
    rep_before = bare.report()
    assert [r[0] for r in rep_before] == ["GPU Culling", "Build HZB", "Lighting", "Sky"]
    s.fresh()
    frame = Frame(hotpath)
    s.set_pass(frame)
    after = _two_frames(s, frame, flags)
    assert frame.report() == rep_before
    for a, b in zip(before, after):
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
    assert (after[1][0] == np.float32(0.625)).all() and not after[1][6].any()
    bare.close(); frame.close()
