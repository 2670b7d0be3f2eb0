"""The render-graph-driven frame on the GPU (csrc/frame/ through include/ur_frame.h): pass order,
pass culling, the bHZBReady hand-over between frames (DeferredRenderer.cpp:519,1210) and parity of the outputs."""
import numpy as np
import pytest

from tests.util import hdr_mismatch

pytestmark = pytest.mark.gpu


def test_frame_passes_and_parity(hotpath, oracle):
    import torch
    from unclerenderer_amd import hostmath, lib, synth
    from unclerenderer_amd.hotpath import Frame, HzbLayout, to_device
    w, h, n = 128, 72, 600
    fc = hostmath.build_frame_constants("sponza", w, h, shadow_size=128, env_mip_count=5)
    g = synth.gbuffer_scene(fc.view, fc.proj, fc.camera_position, w, h, 31)
    shadow, env, lut = synth.shadow_map_noise(128, 31), synth.env_cube_procedural(16, 5), synth.brdf_lut_procedural(64, 16)
    tables = hotpath.make_tables(to_device(shadow), hotpath.stage_env_cube(env, 16, 5), 16, 5, to_device(lut))
    lay = HzbLayout(w, h)
    bounds = synth.instances_random(n, 31, center=fc.camera_position, box=60.0)
    args0 = synth.indirect_args_initial(n)
    dA, dB, dC, dD = to_device(g.A), to_device(g.B), to_device(g.C), to_device(g.depth)
    d_hzb = torch.zeros(lay.total, device="cuda")
    d_args, d_stats = to_device(args0), torch.zeros(2, dtype=torch.int32, device="cuda")
    d_vis, d_cnt = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    consts = hostmath.pack_culling_constants(fc.view, fc.proj, 0, False, 0, 0, 0, True)  # dwords 40-44 are filled by the frame
    frame = Frame(hotpath)

    def render(flags, hdr):
        res = Frame.resources(w, h, 0, h, dA, dB, dC, dD, hdr, dD, d_hzb, lay, tables, to_device(bounds), d_args, n, 0, d_vis, d_cnt, d_stats)
        frame.render(res, consts, fc.scene, fc.sky, flags)
        torch.cuda.synchronize()

    ref_hzb = np.nan_to_num(oracle.build_hzb(g.depth, lay.as_list(), lay.total))
    lit, frag = oracle.deferred_lighting(fc.scene, g.A, g.B, g.C, shadow, env, 16, 5, lut, g.hdr, w, h, want_fragile=True)
    ref_hdr = oracle.sky_atmosphere(fc.sky, g.depth, lit, w, h)

    # ---- frame 1: no HZB yet -> frustum-only cull; HZB is built for the next frame
    assert not frame.hzb_ready
    hdr1 = to_device(g.hdr)
    render(lib.UR_FRAME_DEFAULT, hdr1)
    rep = frame.report()
    assert [r[0] for r in rep] == ["GPU Culling", "Build HZB", "Lighting", "Sky"]
    assert not any(r[1] for r in rep)
    assert frame.hzb_ready
    c_nohzb = hostmath.pack_culling_constants(fc.view, fc.proj, n, False, lay.count, lay.width, lay.height, True)
    ref_args, ref_stats, ref_vis, ref_cnt = oracle.cull_indirect_args(c_nohzb, bounds, None, lay.as_list(), args0)
    assert np.array_equal(d_args.cpu().numpy().view(np.uint32), ref_args)
    assert int(d_cnt.cpu()[0]) == ref_cnt
    assert np.array_equal(d_hzb.cpu().numpy().view(np.uint32), ref_hzb.view(np.uint32))
    nbad, worst, _ = hdr_mismatch(hdr1.cpu().numpy().view(np.uint16), ref_hdr, exclude=frag)
    assert nbad == 0, (nbad, worst)
    # state tracking: Depth DEPTH_WRITE->SRV (Build HZB), then ->DEPTH_READ (Sky); G-buffers RT->PSR; shadow ->PSR
    tr = {r[0]: r[2] for r in rep}
    assert tr["GPU Culling"] == 0 and tr["Build HZB"] == 1 and tr["Lighting"] == 4 and tr["Sky"] == 1

    # ---- frame 2: last frame's HZB drives occlusion culling
    d_args.copy_(to_device(args0)); d_stats.zero_()
    hdr2 = to_device(g.hdr)
    render(lib.UR_FRAME_DEFAULT | lib.UR_FRAME_FUSE_LIGHTING_SKY, hdr2)
    rep = frame.report()
    assert [(r[0], r[1]) for r in rep] == [("GPU Culling", False), ("Build HZB", False), ("Lighting", False), ("Sky", True)]
    c_hzb = hostmath.pack_culling_constants(fc.view, fc.proj, n, True, lay.count, lay.width, lay.height, True)
    ref_args2, ref_stats2, ref_vis2, ref_cnt2 = oracle.cull_indirect_args(c_hzb, bounds, ref_hzb, lay.as_list(), args0)
    assert ref_stats2[1] > 0, "fixture must exercise occlusion"
    assert np.array_equal(d_args.cpu().numpy().view(np.uint32), ref_args2)
    assert np.array_equal(d_vis.cpu().numpy().view(np.uint32)[:ref_cnt2], ref_vis2)
    assert np.array_equal(d_stats.cpu().numpy().view(np.uint32), ref_stats2)
    assert torch.equal(hdr1, hdr2), "fused Lighting+Sky pass must equal Lighting followed by Sky"
    # the Build HZB lambda leaves HZBState = NON_PIXEL_SHADER_RESOURCE (DeferredRenderer.cpp:1209), so the cull pass needs
    # no transition; Build HZB takes it back to UNORDERED_ACCESS and Depth from DEPTH_READ back to an SRV state
    tr = {r[0]: r[2] for r in rep}
    assert tr["GPU Culling"] == 0 and tr["Build HZB"] == 2

    # ---- HZB disabled: the pass is not even added and readiness drops (DeferredRenderer.cpp:514-517)
    render(lib.UR_FRAME_DEFAULT & ~lib.UR_FRAME_HZB, to_device(g.hdr))
    assert [r[0] for r in frame.report()] == ["GPU Culling", "Lighting", "Sky"] and not frame.hzb_ready
    # ---- indirect draw off: the culling pass declares nothing and is culled by the graph
    render(lib.UR_FRAME_DEFAULT & ~lib.UR_FRAME_INDIRECT_DRAW, to_device(g.hdr))
    assert frame.report()[0] == ("GPU Culling", True, 0)
    # ---- async compute: GPU Culling + Build HZB on the second stream give the same words / HZB / HDR
    frame.reset_hzb()
    d_hzb.zero_()
    for k in range(3):
        d_args.copy_(to_device(args0)); d_stats.zero_()
        hdr3 = to_device(g.hdr)
        render(lib.UR_FRAME_DEFAULT | lib.UR_FRAME_FUSE_LIGHTING_SKY | lib.UR_FRAME_ASYNC_COMPUTE, hdr3)
        lanes = {n: a for n, a, _ in frame.report_async()}
        assert lanes["GPU Culling"] and lanes["Build HZB"] and not lanes["Lighting"]
        assert torch.equal(hdr3, hdr1)
        assert np.array_equal(d_hzb.cpu().numpy().view(np.uint32), ref_hzb.view(np.uint32))
        want = ref_args if k == 0 else ref_args2  # first frame after the reset has no HZB yet
        assert np.array_equal(d_args.cpu().numpy().view(np.uint32), want)
    # ---- Tonemap pass appended after Sky (next row): Exposure 0.9, Gamma 2.2, PBR-neutral
    ldr = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    hdr4 = to_device(g.hdr)
    res = Frame.resources(w, h, 0, h, dA, dB, dC, dD, hdr4, dD, d_hzb, lay, tables, to_device(bounds), d_args, n, 0, d_vis, d_cnt, d_stats, tonemap_band=ldr)
    frame.render(res, consts, fc.scene, fc.sky, lib.UR_FRAME_DEFAULT | lib.UR_FRAME_TONEMAP)
    torch.cuda.synchronize()
    assert [r[0] for r in frame.report()] == ["GPU Culling", "Build HZB", "Lighting", "Sky", "Tonemap"]
    ref_ldr = oracle.tonemap(hdr4.cpu().numpy().view(np.uint16), exposure=0.9, gamma=2.2)
    sh8 = np.array([0, 8, 16, 24], np.uint32)
    dl = np.abs(((ldr.cpu().numpy().view(np.uint32)[..., None] >> sh8) & 255).astype(np.int32) - ((ref_ldr[..., None] >> sh8) & 255).astype(np.int32))
    assert dl.max() <= 1
    # ---- GPU timing: event pairs per pass, harvested when the slot comes round again
    for _ in range(8):
        render(lib.UR_FRAME_DEFAULT | lib.UR_FRAME_GPU_TIMING, to_device(g.hdr))
    names = {t[0] for t in frame.timing_stats()}
    assert {"GPU Culling", "Build HZB", "Lighting", "Sky"} <= names
    frame.close()


def test_lighting_timing_forms_leave_the_frame_alone(hotpath):
    """The three ways a Lighting pass is timed — an event bracket on the stream (UR_FRAME_TIME_LIGHTING), the pair carried on the
    Lighting dispatch (UR_FRAME_TIME_LIGHTING_KERNEL: begin = the end of the cull dispatch in front when the frame is exactly those
    two launches, ur_time_next_cull), and ur_time_next_lighting called directly — report positive durations of the same order
    and change no byte of the frame."""
    import torch
    from unclerenderer_amd import hostmath, lib, synth
    from unclerenderer_amd.hotpath import Frame, HzbLayout, to_device
    w, h, n = 256, 144, 300
    fc = hostmath.build_frame_constants("sponza", w, h, shadow_size=128, env_mip_count=5)
    g = synth.gbuffer_scene(fc.view, fc.proj, fc.camera_position, w, h, 37)
    shadow, env, lut = synth.shadow_map_noise(128, 37), synth.env_cube_procedural(16, 5), synth.brdf_lut_procedural(64, 16)
    tables = hotpath.make_tables(to_device(shadow), hotpath.stage_env_cube(env, 16, 5), 16, 5, to_device(lut))
    lay = HzbLayout(w, h)
    bounds = to_device(synth.instances_random(n, 37, center=fc.camera_position, box=60.0))
    args0 = synth.indirect_args_initial(n)
    dA, dB, dC, dD = to_device(g.A), to_device(g.B), to_device(g.C), to_device(g.depth)
    consts = hostmath.pack_culling_constants(fc.view, fc.proj, 0, False, 0, 0, 0, True)
    base = lib.UR_FRAME_DEFAULT | lib.UR_FRAME_FUSE_LIGHTING_SKY

    def run(flags, frames=6, with_list=True):
        frame = Frame(hotpath)
        d_hzb = torch.zeros(lay.total, device="cuda")
        d_args, d_stats = to_device(args0), torch.zeros(2, dtype=torch.int32, device="cuda")
        d_vis, d_cnt = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
        hdr = None
        for _ in range(frames):
            d_args.copy_(to_device(args0)); d_stats.zero_()
            hdr = to_device(g.hdr)
            res = Frame.resources(w, h, 0, h, dA, dB, dC, dD, hdr, dD, d_hzb, lay, tables, bounds, d_args, n, 0, d_vis if with_list else None,
                                  d_cnt if with_list else None, d_stats)
            frame.render(res, consts, fc.scene, fc.sky, flags)
        torch.cuda.synchronize()
        times = frame.lighting_times_ms()
        frame.close()
        return (hdr.cpu(), d_hzb.cpu(), d_args.cpu(), d_vis.cpu(), d_cnt.cpu(), d_stats.cpu()), times

    for ride in (0, lib.UR_FRAME_HZB_WITH_LIGHTING):  # separate Build HZB launches / the chain riding in the Lighting launch
        ref, t0 = run(base | ride)
        assert t0.size == 0
        for timed in (lib.UR_FRAME_TIME_LIGHTING, lib.UR_FRAME_TIME_LIGHTING_KERNEL):
            out, t = run(base | ride | timed)
            assert t.size == 6 and (t > 0).all() and (t < 5.0).all(), (ride, timed, t)
            for a, b in zip(ref, out):
                assert torch.equal(a, b), (ride, timed)
    # more than 256 commands and NO visible list: the cull is one multi-workgroup launch, which carries the start event itself
    # (round 3 left the event in the context on this path and the sample read a stale stamp)
    ref, _ = run(base | lib.UR_FRAME_HZB_WITH_LIGHTING, with_list=False)
    out, t = run(base | lib.UR_FRAME_HZB_WITH_LIGHTING | lib.UR_FRAME_TIME_LIGHTING_KERNEL, with_list=False)
    assert t.size == 6 and (t > 0).all() and (t < 5.0).all(), t
    for a, b in zip(ref, out):
        assert torch.equal(a, b)

    # the entry point itself: the pair rides on the next Lighting dispatch and is consumed by it
    hdr = to_device(g.hdr)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); e1.record()  # (torch creates the HIP event at the first record)
    torch.cuda.synchronize()
    hotpath.time_next_lighting(e0, e1)
    hotpath.deferred_lighting_sky(fc.scene, fc.sky, dA, dB, dC, dD, tables, hdr, w, h)
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1)
    assert 0.0 < ms < 5.0
    hdr_b = to_device(g.hdr)
    hotpath.deferred_lighting_sky(fc.scene, fc.sky, dA, dB, dC, dD, tables, hdr_b, w, h)  # consumed: this launch carries nothing
    torch.cuda.synchronize()
    assert torch.equal(hdr, hdr_b)
    assert abs(e0.elapsed_time(e1) - ms) < 1e-6
    # a stop event is required when a start event is given
    L = hotpath._L
    import ctypes as C
    assert L.ur_time_next_lighting(hotpath._ctx, C.c_void_p(e0.cuda_event), None) == lib.UR_EINVAL
    assert L.ur_time_next_cull(hotpath._ctx, None) == lib.UR_OK  # NULL is the clearing form (include/ur_hotpath.h)
    hotpath.time_next_lighting(None, None)
    # ur_time_next_cull is consumed or cleared by the very next cull call, whatever that call launches
    c300 = hostmath.pack_culling_constants(fc.view, fc.proj, n, False, 0, 0, 0, False)
    d_args = to_device(args0)
    d_vis, d_cnt = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    for label, cc, vis, cnt, carried in (("words only, two workgroups", c300, None, None, 1), ("with the list", c300, d_vis, d_cnt, 1),
                                         ("no instances, count zeroed", hostmath.pack_culling_constants(fc.view, fc.proj, 0, False, 0, 0, 0, False), d_vis, d_cnt, 1),
                                         ("no instances, nothing launched", hostmath.pack_culling_constants(fc.view, fc.proj, 0, False, 0, 0, 0, False), None, None, 0)):
        c0, c1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        c0.record(); c1.record()
        torch.cuda.synchronize()
        assert L.ur_time_next_cull(hotpath._ctx, C.c_void_p(c0.cuda_event)) == lib.UR_OK
        assert L.ur_time_cull_carried(hotpath._ctx) == 0
        hotpath.cull_indirect_args(cc, bounds, None, None, d_args, None, vis, cnt)
        assert L.ur_time_cull_carried(hotpath._ctx) == carried, label
        hotpath.time_next_lighting(None, c1)
        hotpath.deferred_lighting_sky(fc.scene, fc.sky, dA, dB, dC, dD, tables, hdr_b, w, h)
        torch.cuda.synchronize()
        if carried:
            assert 0.0 < c0.elapsed_time(c1) < 5.0, label  # end of the cull call's last dispatch -> end of the Lighting dispatch
        # the event did not stay behind: a second cull carries nothing
        hotpath.cull_indirect_args(c300, bounds, None, None, d_args, None, None, None)
        assert L.ur_time_cull_carried(hotpath._ctx) == 0, label
