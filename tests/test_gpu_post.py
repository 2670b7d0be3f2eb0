"""AutoExposure, CAS and the fused Tonemap+CAS launch on the GPU (csrc/post.hip), against the scalar restatement of the HLSL
(tests/post_ref.py), against each other, and wired into the frame (UR_FRAME_AUTO_EXPOSURE / CAS / FUSE_TONEMAP_CAS)."""
import numpy as np
import pytest

from tests import post_ref

pytestmark = pytest.mark.gpu

SIZES_AE = [(1080, 1920), (2160, 3840), (131, 257), (9, 17)]


def _torch():
    import torch
    return torch


def _hdr_bits(h, w, seed, scale=1.0):
    """(h, w, 4) uint16 RGBA16F: a smooth gradient times noise with a wide range of luminance."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    base = 0.05 + 2.0 * (x / max(w - 1, 1)) * (y / max(h - 1, 1))
    hdr = np.zeros((h, w, 4), np.float16)
    hdr[..., :3] = np.minimum(base[..., None] * (rng.random((h, w, 3)) ** 2 * 3.0) * scale, 60000).astype(np.float16)
    hdr[..., 3] = 1.0
    return hdr.view(np.uint16)


def _ldr(h, w, seed):
    rng = np.random.default_rng(seed)
    b = rng.integers(0, 256, (h, w, 3)).astype(np.uint32)
    b[: h // 2] = (b[: h // 2] // 32) * 32 + 16  # flat-ish and noisy regions
    return (b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16) | np.uint32(0xFF000000)).astype(np.uint32)


def _lsb(a, b):
    return int(np.abs(post_ref.bytes_of(a).astype(np.int32) - post_ref.bytes_of(b).astype(np.int32)).max())


def _assert_cas_bytes(got, ref, what):
    """At most one LSB anywhere, and (like test_tonemap_parity) fewer than 2e-3 of the bytes off at all; an image of fewer than
    500 pixels may have one byte off."""
    d = np.abs(post_ref.bytes_of(got).astype(np.int32) - post_ref.bytes_of(ref).astype(np.int32))
    n = int((d > 0).sum())
    assert d.max() <= 1, (what, int(d.max()))
    assert n < 2e-3 * d.size or (got.size < 500 and n <= 1), (what, n, d.size)


def _ev(hotpath, d_hdr, w, h, **kw):
    torch = _torch()
    out = torch.full((1,), float("nan"), device="cuda")
    hotpath.auto_exposure(d_hdr, out, w, h, **kw)
    torch.cuda.synchronize()
    return float(out.cpu()[0])


@pytest.mark.parametrize("h,w", SIZES_AE)
def test_auto_exposure_against_the_restatement(hotpath, oracle, h, w):
    torch = _torch()
    from unclerenderer_amd.hotpath import to_device
    bits = _hdr_bits(h, w, 11)
    ref_img = post_ref.half4(bits)
    d = to_device(bits)
    target = post_ref.auto_exposure(ref_img)
    got = _ev(hotpath, d, w, h)
    assert abs(got - float(target)) <= 1e-4, (got, target)
    assert np.log2(0.1) < target < np.log2(5.0), "fixture must not sit on a clamp bound"
    # history in both speed directions
    for prev in (float(target) - 1.5, float(target) + 1.5):
        d_prev = torch.tensor([prev], device="cuda")
        kw = dict(use_history=True, delta_time=1 / 30, speed_up=3.0, speed_down=1.0)
        got = _ev(hotpath, d, w, h, prev_ev=d_prev, **kw)
        want = post_ref.auto_exposure(ref_img, prev=np.float32(prev), **kw)
        assert abs(got - float(want)) <= 1e-4, (prev, got, want)
        assert (want > prev) == (prev < target)
    # each clamp bound
    for scale, bound in ((1000.0, np.log2(np.float32(0.1))), (1e-4, np.log2(np.float32(5.0)))):
        sb = _hdr_bits(h, w, 12, scale)
        assert post_ref.auto_exposure(post_ref.half4(sb)) == bound
        assert abs(_ev(hotpath, to_device(sb), w, h) - float(bound)) <= 1e-4
    # a NaN texel inside the footprint of lane (0, 0): t = size / 32 - 0.5
    nb = bits.copy().view(np.float16)
    ty, tx = int(np.floor(np.float32(h) / 32 - 0.5)), int(np.floor(np.float32(w) / 32 - 0.5))
    nb[min(max(ty, 0), h - 1), min(max(tx, 0), w - 1), 1] = np.nan
    nb = nb.view(np.uint16)
    want = post_ref.auto_exposure(post_ref.half4(nb))
    assert want != target and np.isfinite(want)
    assert abs(_ev(hotpath, to_device(nb), w, h) - float(want)) <= 1e-4
    # the same input gives the same bits
    a, b = torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda")
    hotpath.auto_exposure(d, a, w, h)
    hotpath.auto_exposure(d, b, w, h)
    torch.cuda.synchronize()
    assert a.cpu().numpy().view(np.uint32)[0] == b.cpu().numpy().view(np.uint32)[0]
    # the EV drives Tonemap: within one LSB of the oracle's Tonemap at that EV
    if h * w <= 1920 * 1080:
        ev = float(a.cpu()[0])
        out = torch.zeros((h, w), dtype=torch.int32, device="cuda")
        hotpath.tonemap(d, out, w, h, exposure=0.9, gamma=2.2, exposure_ev=a)
        ref = oracle.tonemap(bits, exposure=0.9, gamma=2.2, exposure_ev=ev)
        assert _lsb(out.cpu().numpy().view(np.uint32), ref) <= 1


def test_auto_exposure_argument_checks(hotpath):
    import ctypes as C
    from unclerenderer_amd import lib
    from unclerenderer_amd.hotpath import to_device
    torch = _torch()
    d = to_device(_hdr_bits(9, 17, 1))
    out = torch.zeros(1, device="cuda")
    L, ctx = hotpath._L, hotpath.ctx
    k = lib.AutoExposureConstants((C.c_float * 2)(17, 9), 0.0, 3.0, 1.0, 0, 0.3, 0.1, 5.0)
    p = lambda t: C.c_void_p(t.data_ptr())
    assert L.ur_auto_exposure(ctx, None, p(d), 17, 9, None, p(out)) == lib.UR_EINVAL
    assert L.ur_auto_exposure(ctx, C.byref(k), p(d), 17, 8, None, p(out)) == lib.UR_EINVAL  # InputSize != (w, h)
    assert L.ur_auto_exposure(ctx, C.byref(k), p(d), 0, 9, None, p(out)) == lib.UR_EINVAL
    k.UseHistory = 1
    assert L.ur_auto_exposure(ctx, C.byref(k), p(d), 17, 9, None, p(out)) == lib.UR_EINVAL  # history without prev
    assert L.ur_auto_exposure(ctx, C.byref(k), p(d), 17, 9, p(out), p(out)) == lib.UR_OK    # prev may be out
    torch.cuda.synchronize()


CAS_SIZES = [(1080, 1920), (131, 257), (64, 128), (9, 17), (1, 37), (37, 1), (1, 1), (2, 2)]


@pytest.mark.parametrize("h,w", CAS_SIZES)
def test_cas_against_the_restatement(hotpath, h, w):
    torch = _torch()
    from unclerenderer_amd.hotpath import to_device
    img = _ldr(h, w, h * 1000 + w)
    d = to_device(img)
    for s in (0.0, 0.5, 1.0):
        ref = post_ref.cas(img, s)
        out = torch.zeros((h, w), dtype=torch.int32, device="cuda")
        hotpath.cas(d, out, w, h, sharpness=s)
        torch.cuda.synchronize()
        full = out.cpu().numpy().view(np.uint32)
        _assert_cas_bytes(full, ref, s)
        if s == 0.0:
            assert np.array_equal(full, img)
        # bands: first row, middle, last row, 1-row bands; stacked they are the full frame, bit for bit
        cuts = sorted({0, min(1, h), h // 3, h // 2, max(h - 1, 0), h})
        stacked = torch.zeros((h, w), dtype=torch.int32, device="cuda")
        for r0, r1 in zip(cuts[:-1], cuts[1:]):
            if r1 > r0:
                hotpath.cas(d, stacked[r0:r1], w, h, row0=r0, rows=r1 - r0, sharpness=s)
        torch.cuda.synchronize()
        assert torch.equal(stacked, out)
        # the one-pixel-per-lane form (input only 4-byte aligned) gives the same bits
        shifted = torch.zeros(h * w + 1, dtype=torch.int32, device="cuda")
        shifted[1:] = d.reshape(-1)
        out1 = torch.zeros((h, w), dtype=torch.int32, device="cuda")
        hotpath.cas(shifted[1:], out1, w, h, sharpness=s)
        torch.cuda.synchronize()
        assert torch.equal(out1, out)


@pytest.mark.parametrize("s", [0.5, 1.0])
def test_cas_8k_against_the_restatement(hotpath, s):
    """7680x4320 against the restatement, compared in bands of 540 rows (each band's restatement reads its halo rows from the
    whole image); the fused Tonemap+CAS launch is byte-equal to the two launches (test_tonemap_cas_equals_tonemap_then_cas), so this
    covers it too."""
    torch = _torch()
    from unclerenderer_amd.hotpath import to_device
    h, w = 4320, 7680
    img = _ldr(h, w, 4320 * 1000 + 7680)
    d = to_device(img)
    out = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    hotpath.cas(d, out, w, h, sharpness=s)
    torch.cuda.synchronize()
    full = out.cpu().numpy().view(np.uint32)
    for r0 in range(0, h, 540):
        _assert_cas_bytes(full[r0:r0 + 540], post_ref.cas(img, s, r0, 540), (s, r0))


def test_cas_argument_checks(hotpath):
    import ctypes as C
    from unclerenderer_amd import lib
    torch = _torch()
    d = torch.zeros((9, 17), dtype=torch.int32, device="cuda")
    out = torch.zeros((9, 17), dtype=torch.int32, device="cuda")
    L, ctx = hotpath._L, hotpath.ctx
    p = lambda t: C.c_void_p(t.data_ptr())
    k = lib.CasConstants((C.c_float * 2)(1 / 17, 1 / 9), 0.5, 0.0)
    assert L.ur_cas(ctx, None, p(d), p(out), 17, 9, 0, 9) == lib.UR_EINVAL
    assert L.ur_cas(ctx, C.byref(k), p(d), p(out), 17, 9, 0, 0) == lib.UR_EINVAL   # empty band
    assert L.ur_cas(ctx, C.byref(k), p(d), p(out), 17, 9, 5, 5) == lib.UR_EINVAL   # past the frame
    assert L.ur_cas(ctx, C.byref(k), p(d), p(d), 17, 9, 0, 9) == lib.UR_EINVAL     # in place
    k2 = lib.CasConstants((C.c_float * 2)(0.5 / 17, 1 / 9), 0.5, 0.0)
    assert L.ur_cas(ctx, C.byref(k2), p(d), p(out), 17, 9, 0, 9) == lib.UR_EUNSUPPORTED  # not one texel
    tk = lib.TonemapConstants(1, 0, 1.0, 2.2)
    assert L.ur_tonemap_cas(ctx, C.byref(tk), None, p(d), None, p(out), 17, 9, 0, 9) == lib.UR_EINVAL
    assert L.ur_tonemap_cas(ctx, C.byref(tk), C.byref(k), p(d), None, p(out), 17, 9, 9, 1) == lib.UR_EINVAL
    torch.cuda.synchronize()


FUSED_SIZES = [(1080, 1920), (2160, 3840), (4320, 7680), (131, 257), (9, 17), (1, 1), (2, 2), (3, 1), (1, 6)]


@pytest.mark.parametrize("h,w", FUSED_SIZES)
def test_tonemap_cas_equals_tonemap_then_cas(hotpath, h, w):
    torch = _torch()
    from unclerenderer_amd.hotpath import to_device
    d = to_device(_hdr_bits(h, w, 7))
    ev = torch.tensor([-0.75], device="cuda")
    ldr = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    two = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    one = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    for kw in (dict(exposure=0.9), dict(exposure=0.9, enable_tonemap=False), dict(exposure=2.0, exposure_ev=ev)):
        for s in (0.5, 1.0):
            hotpath.tonemap(d, ldr, w, h, gamma=2.2, **kw)
            hotpath.cas(ldr, two, w, h, sharpness=s)
            one.fill_(0)
            hotpath.tonemap_cas(d, one, w, h, gamma=2.2, sharpness=s, **kw)
            torch.cuda.synchronize()
            assert torch.equal(one, two), (kw, s)
        if h >= 3:  # bands: the first rows, a middle one, the last row
            for r0, n in ((0, 2), (h // 2, 1), (h - 1, 1), (1, h - 2)):
                band = torch.zeros((n, w), dtype=torch.int32, device="cuda")
                hotpath.tonemap_cas(d, band, w, h, row0=r0, rows=n, gamma=2.2, sharpness=1.0, **kw)
                hotpath.cas(ldr, two, w, h, sharpness=1.0)
                torch.cuda.synchronize()
                assert torch.equal(band, two[r0:r0 + n]), (kw, r0, n)
    if h * w <= 1920 * 1080:  # the one-pixel-per-lane form (HDR only 8-byte aligned)
        shifted = torch.zeros(h * w * 4 + 4, dtype=torch.int16, device="cuda")
        shifted[4:] = d.reshape(-1)
        hotpath.tonemap_cas(shifted[4:], one, w, h, exposure=0.9, gamma=2.2, sharpness=0.5)
        hotpath.tonemap(d, ldr, w, h, exposure=0.9, gamma=2.2)
        hotpath.cas(ldr, two, w, h, sharpness=0.5)
        torch.cuda.synchronize()
        assert torch.equal(one, two)


# ---- the frame ---------------------------------------------------------------------------------------------------------------

def test_frame_post_chain(hotpath):
    torch = _torch()
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
    consts = hostmath.pack_culling_constants(fc.view, fc.proj, 0, False, 0, 0, 0, True)
    frame = Frame(hotpath)
    lum = (torch.full((1,), float("nan"), device="cuda"), torch.full((1,), float("nan"), device="cuda"))
    scratch = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    ldr = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    AE, CAS, FUSE = lib.UR_FRAME_AUTO_EXPOSURE, lib.UR_FRAME_CAS, lib.UR_FRAME_FUSE_TONEMAP_CAS
    base = lib.UR_FRAME_DEFAULT | lib.UR_FRAME_TONEMAP

    def render(flags, rows=h, band=ldr):
        hdr = to_device(g.hdr)
        d_args.copy_(to_device(args0))
        res = Frame.resources(w, h, 0, rows, dA, dB, dC, dD, hdr, dD, d_hzb, lay, tables, to_device(bounds), d_args, n, 0, d_vis, d_cnt,
                              d_stats, tonemap_band=band)
        frame.render(res, consts, fc.scene, fc.sky, flags)
        torch.cuda.synchronize()
        return hdr

    # by hand: the standalone calls with the reference's ping-pong (DeferredRenderer.cpp:1363-1573, 1612-1620)
    ref_lum = [torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda")]
    state = {"w": 0, "valid": False}

    def by_hand(hdr, dt, ae=True, cas=True):
        r_ldr = torch.zeros((h, w), dtype=torch.int32, device="cuda")
        tmp = torch.zeros((h, w), dtype=torch.int32, device="cuda")
        ev = None
        if ae:
            W = state["w"]
            hotpath.auto_exposure(hdr, ref_lum[W], w, h, prev_ev=ref_lum[1 - W] if state["valid"] else None, use_history=state["valid"],
                                  delta_time=dt)
            ev = ref_lum[W]
        hotpath.tonemap(hdr, tmp if cas else r_ldr, w, h, exposure=0.9, gamma=2.2, exposure_ev=ev)
        if cas:
            hotpath.cas(tmp, r_ldr, w, h, sharpness=0.5)
        torch.cuda.synchronize()
        if ae:
            state["valid"], state["w"] = True, 1 - state["w"]
        else:
            state["valid"] = False
        return r_ldr

    def bits(t):
        return int(t.cpu().numpy().view(np.uint32)[0])

    def poison(v):
        """The texel the next AutoExposure pass reads as history gets v (the frame's copy and the hand-chained one alike): every frame
        re-lights the same G-buffer, so without this the history would already hold the frame's target and adapting would not move it."""
        W = state["w"]
        lum[1 - W].fill_(v)
        ref_lum[1 - W].fill_(v)

    free = torch.zeros(1, device="cuda")

    def ev_with(hdr, prev=None, dt=0.0):
        """This HDR's EV without history (prev None) or adapted from prev over dt, by the standalone call."""
        if prev is None:
            hotpath.auto_exposure(hdr, free, w, h)
        else:
            hotpath.auto_exposure(hdr, free, w, h, prev_ev=torch.tensor([prev], device="cuda"), use_history=True, delta_time=dt)
        torch.cuda.synchronize()
        return bits(free)

    names = ["GPU Culling", "Build HZB", "Lighting", "Sky", "AutoExposure", "Tonemap", "CAS"]
    T = None  # the frame's target EV (the same HDR every frame)
    for k, dt in enumerate((1 / 60, 1 / 30, 1 / 45)):
        frame.set_post(luminance=lum, tonemap_scratch=scratch, delta_time=dt)
        W = state["w"]
        # frame 1 has no history; frames 2 and 3 adapt from a texel above, then below the target (speed down, then up)
        poison(3.0 if T is None else T + (1.5 if k == 1 else -1.5))
        hdr = render(base | AE | CAS)
        assert [r[0] for r in frame.report()] == names
        assert not any(r[1] for r in frame.report())
        want = by_hand(hdr, dt)
        assert bits(lum[W]) == bits(ref_lum[W]), k
        assert torch.equal(ldr, want), k
        if T is None:
            assert bits(lum[W]) == ev_with(hdr)  # UseHistory = 0
            T = float(lum[W].cpu()[0])
        else:
            prev = float(lum[1 - W].cpu()[0])
            assert bits(lum[W]) == ev_with(hdr, prev, dt) != ev_with(hdr)  # adapted with this frame's DeltaTime
            assert bits(lum[W]) != ev_with(hdr, prev, 2 * dt)
            got = float(lum[W].cpu()[0])
            assert min(prev, T) < got < max(prev, T)
    # fused: the same bytes, CAS culled
    poison(T - 1.5)
    hdr = render(base | AE | CAS | FUSE)
    assert [(r[0], r[1]) for r in frame.report()] == [(nm, nm == "CAS") for nm in names]
    assert torch.equal(ldr, by_hand(hdr, 1 / 45))
    # after ur_frame_reset_post the next AutoExposure has no history: its EV is the target, not the value adapted from the texel
    frame.reset_post()
    state["valid"] = False
    W = state["w"]
    poison(T + 1.5)
    hdr = render(base | AE | CAS)
    assert torch.equal(ldr, by_hand(hdr, 1 / 45))
    assert bits(lum[W]) == ev_with(hdr) != ev_with(hdr, T + 1.5, 1 / 45)
    # a frame without AutoExposure drops the history too
    hdr = render(base | CAS)
    assert [r[0] for r in frame.report()] == ["GPU Culling", "Build HZB", "Lighting", "Sky", "Tonemap", "CAS"]
    assert torch.equal(ldr, by_hand(hdr, 1 / 45, ae=False))
    W = state["w"]
    poison(T - 1.5)
    hdr = render(base | AE | CAS | FUSE)
    assert torch.equal(ldr, by_hand(hdr, 1 / 45))
    assert bits(lum[W]) == bits(ref_lum[W]) == ev_with(hdr) != ev_with(hdr, T - 1.5, 1 / 45)
    # ... and the frame after it adapts again
    poison(T + 1.5)
    hdr = render(base | AE | CAS)
    assert torch.equal(ldr, by_hand(hdr, 1 / 45))
    assert bits(lum[1 - W]) == ev_with(hdr, T + 1.5, 1 / 45)
    # a band of the frame: AutoExposure / CAS need the whole frame
    for fl in (base | AE, base | CAS, base | CAS | FUSE):
        with pytest.raises(lib.UrError) as e:
            render(fl, rows=h // 2, band=ldr[: h // 2])
        assert e.value.code == lib.UR_EUNSUPPORTED
    # without UR_FRAME_TONEMAP / a tonemap band
    for fl, band in ((lib.UR_FRAME_DEFAULT | AE, ldr), (base | CAS, None)):
        with pytest.raises(lib.UrError) as e:
            render(fl, band=band)
        assert e.value.code == lib.UR_EINVAL
    # Tonemap alone: today's pass, today's bytes
    hdr = render(base)
    assert [r[0] for r in frame.report()] == ["GPU Culling", "Build HZB", "Lighting", "Sky", "Tonemap"]
    plain = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    hotpath.tonemap(hdr, plain, w, h, exposure=0.9, gamma=2.2)
    torch.cuda.synchronize()
    assert torch.equal(ldr, plain)
    frame.close()
