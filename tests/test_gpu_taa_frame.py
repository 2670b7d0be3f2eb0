"""TemporalAA in the frame on the GPU: the fused TemporalAA + Tonemap launch against the two launches and the oracle, the frame's
history ring / jitter sequence rebuilt from the oracle alone, and that nothing else in the frame moved."""
import numpy as np
import pytest

from tests import post_ref

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A  # fp16 205.25 in every channel: no frame here produces it


def _torch():
    import torch
    return torch


def _lsb(a, b):
    return int(np.abs(post_ref.bytes_of(a).astype(np.int32) - post_ref.bytes_of(b).astype(np.int32)).max())


def _assert_tonemap_bytes(got, ref, what):
    """The project's Tonemap criterion against the oracle (tests/test_gpu_post.py, test_tonemap_parity): at most one LSB anywhere
    and fewer than 2e-3 of the bytes off at all. Prints the figures first."""
    d = np.abs(post_ref.bytes_of(got).astype(np.int32) - post_ref.bytes_of(ref).astype(np.int32))
    n = int((d > 0).sum())
    print(f"{what}: max LSB {_lsb(got, ref)}, bytes off {n} of {d.size} ({n / d.size:.2e})")
    assert d.max() <= 1, (what, int(d.max()))
    assert n < 2e-3 * d.size, (what, n, d.size)


def _taa_frames(h, w, seed):
    rng = np.random.default_rng(seed)
    cur = (rng.random((h, w, 4), np.float32) ** 2 * 8).astype(np.float16)
    hist = (rng.random((h, w, 4), np.float32) ** 2 * 8).astype(np.float16)
    cur[..., 3] = 2.0
    return cur.view(np.uint16), hist.view(np.uint16)


def _u16(t):
    return t.cpu().numpy().view(np.uint16)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


# ---- the fused launch ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h,w", [(1080, 1920), (2160, 3840), (67, 515), (9, 130)])
def test_fused_equals_two_launches_equals_oracle(hotpath, oracle, h, w):
    """history_out byte-equal to oracle.temporal_aa and to ur_temporal_aa; the LDR image byte-equal to ur_tonemap of that image and
    within the Tonemap criterion of oracle.tonemap of it; use_history 0 and 1, with and without an EV, whole frame and bands, either
    history-store hint, and with the history read and written in place (a ring of one image)."""
    torch = _torch()
    from unclerenderer_amd import lib
    from unclerenderer_amd.hotpath import to_device
    cb, hb = _taa_frames(h, w, 5 * h + w)
    d_cur, d_hist = to_device(cb), to_device(hb)
    ev = torch.tensor([-0.75], device="cuda")
    for use in (False, True):
        ref_hist = oracle.temporal_aa(cb, hb, 0.9, use)
        two_hist = torch.zeros((h, w, 4), dtype=torch.int16, device="cuda")
        hotpath.temporal_aa(d_cur, d_hist, two_hist, 0.9, use, w, h)
        for kw, okw in ((dict(exposure=0.9), dict(exposure=0.9)), (dict(exposure=2.0, exposure_ev=ev), dict(exposure=2.0, exposure_ev=-0.75))):
            what = f"{w}x{h} use={int(use)} ev={'exposure_ev' in kw}"
            two_ldr = torch.zeros((h, w), dtype=torch.int32, device="cuda")
            hotpath.tonemap(two_hist, two_ldr, w, h, gamma=2.2, **kw)
            one_hist = torch.full((h, w, 4), SENTINEL, dtype=torch.int16, device="cuda")
            one_ldr = torch.zeros((h, w), dtype=torch.int32, device="cuda")
            hotpath.temporal_aa_tonemap(d_cur, d_hist, one_hist, one_ldr, 0.9, use, w, h, gamma=2.2, **kw)
            torch.cuda.synchronize()
            assert np.array_equal(_u16(one_hist), ref_hist), what
            assert torch.equal(one_hist, two_hist), what
            assert torch.equal(one_ldr, two_ldr), what
            _assert_tonemap_bytes(_u32(one_ldr), oracle.tonemap(ref_hist, gamma=2.2, **okw), what)
            # bands off the 8-row grid: the first rows, one middle row, the last rows, all but the edge rows
            for r0, n in ((0, 3), (h // 2 + 1, 1), (h - 5, 5), (1, h - 2)):
                bh = torch.full((n, w, 4), SENTINEL, dtype=torch.int16, device="cuda")
                bl = torch.zeros((n, w), dtype=torch.int32, device="cuda")
                hotpath.temporal_aa_tonemap(d_cur, d_hist[r0:r0 + n], bh, bl, 0.9, use, w, h, r0, n, gamma=2.2, **kw)
                torch.cuda.synchronize()
                assert torch.equal(bh, two_hist[r0:r0 + n]) and torch.equal(bl, two_ldr[r0:r0 + n]), (what, r0, n)
        # the plain history store: the same bytes
        hotpath.set_option(lib.UR_OPT_TAA_TONEMAP_HISTORY_STORE, 1)
        try:
            one_hist.fill_(SENTINEL)
            one_ldr.zero_()
            hotpath.temporal_aa_tonemap(d_cur, d_hist, one_hist, one_ldr, 0.9, use, w, h, gamma=2.2, exposure=2.0, exposure_ev=ev)
            torch.cuda.synchronize()
        finally:
            hotpath.set_option(lib.UR_OPT_TAA_TONEMAP_HISTORY_STORE, 0)
        assert torch.equal(one_hist, two_hist) and torch.equal(one_ldr, two_ldr), (w, h, use)
        # a ring of one image: history read and written in place, by both entry points
        for fused in (False, True):
            inplace = d_hist.clone()
            if fused:
                one_ldr.zero_()
                hotpath.temporal_aa_tonemap(d_cur, inplace, inplace, one_ldr, 0.9, use, w, h, gamma=2.2, exposure=2.0, exposure_ev=ev)
            else:
                hotpath.temporal_aa(d_cur, inplace, inplace, 0.9, use, w, h)
            torch.cuda.synchronize()
            assert np.array_equal(_u16(inplace), ref_hist), (w, h, use, fused)
            assert not fused or torch.equal(one_ldr, two_ldr)


TAA_SPECIAL = [0x7E00, 0x7D00, 0xFD00, 0x7E01, 0x0000, 0x8000, 0x0001, 0x8001, 0x03FF, 0x7C00, 0xFC00]


def test_fused_special_values_in_every_position(hotpath, oracle):
    """The special values of test_temporal_aa_special_values_in_every_position (quiet and signalling NaN patterns, +-0, subnormals,
    +-Inf in the centre, in the columns around a wave, in the halo rows of a strip, at the frame edges and in the history) through the
    fused launch: the history is the oracle's (a NaN result is a NaN in both; its sign and payload are the hardware's, as in that
    test), the LDR bytes are ur_tonemap's of that image and pass the Tonemap criterion against oracle.tonemap of it."""
    torch = _torch()
    from unclerenderer_amd.hotpath import to_device
    h, w = 26, 200
    cur, hist = _taa_frames(h, w, 3)
    cols = [0, 1, 62, 63, 64, 65, 126, 127, 128, 129, 191, 199]
    rows = [0, 1, 6, 7, 8, 9, 15, 16, 24, 25]
    k = 0
    for y in rows:
        for x in cols:
            v = TAA_SPECIAL[k % len(TAA_SPECIAL)]
            ch = k % 3
            cur[y, x, ch] = v
            if k % 4 == 0:
                cur[y, x, :3] = v
            if k % 5 == 0:
                hist[(y + 3) % h, (x + 7) % w, ch] = TAA_SPECIAL[(k + 3) % len(TAA_SPECIAL)]
            k += 1
    cur[20, 64, :3] = 0x7D00
    cur[20, 62, 2] = 0xFC00
    cur[19, 63, 2] = np.float16(6.5).view(np.uint16)
    hist[19, 63, 2] = np.float16(0.25).view(np.uint16)
    d_cur, d_hist = to_device(cur), to_device(hist)
    ev = torch.tensor([0.5], device="cuda")
    for wt in (0.9, 0.35, 1.0, 0.0):
        for use in (True, False):
            one_hist = torch.full((h, w, 4), SENTINEL, dtype=torch.int16, device="cuda")
            one_ldr = torch.zeros((h, w), dtype=torch.int32, device="cuda")
            two_hist, two_ldr = torch.zeros_like(one_hist), torch.zeros_like(one_ldr)
            hotpath.temporal_aa_tonemap(d_cur, d_hist, one_hist, one_ldr, wt, use, w, h, exposure=0.9, gamma=2.2, exposure_ev=ev)
            hotpath.temporal_aa(d_cur, d_hist, two_hist, wt, use, w, h)
            hotpath.tonemap(two_hist, two_ldr, w, h, exposure=0.9, gamma=2.2, exposure_ev=ev)
            torch.cuda.synchronize()
            got, ref = _u16(one_hist), oracle.temporal_aa(cur, hist, wt, use)
            nan_g, nan_r = np.isnan(got.view(np.float16)), np.isnan(ref.view(np.float16))
            assert np.array_equal(nan_g, nan_r), (wt, use)
            bad = np.argwhere((got != ref) & ~nan_r)
            assert len(bad) == 0, (wt, use, [(tuple(b), hex(got[tuple(b)]), hex(ref[tuple(b)])) for b in bad[:6]])
            assert torch.equal(one_hist, two_hist) and torch.equal(one_ldr, two_ldr), (wt, use)
            _assert_tonemap_bytes(_u32(one_ldr), oracle.tonemap(got, exposure=0.9, gamma=2.2, exposure_ev=0.5), f"special wt={wt} use={int(use)}")


# ---- the frame -----------------------------------------------------------------------------------------------------------------

class _Scene:
    """A small frame's inputs: a G-buffer per seed (a different Lighting image each frame) and everything else fixed."""

    def __init__(self, hotpath, w=128, h=72, n=600):
        torch = _torch()
        from unclerenderer_amd import hostmath, synth
        from unclerenderer_amd.hotpath import HzbLayout, to_device
        self.hp, self.w, self.h, self.n = hotpath, w, h, n
        self.fc = hostmath.build_frame_constants("sponza", w, h, shadow_size=128, env_mip_count=5)
        shadow, env, lut = synth.shadow_map_noise(128, 31), synth.env_cube_procedural(16, 5), synth.brdf_lut_procedural(64, 16)
        self.tables = hotpath.make_tables(to_device(shadow), hotpath.stage_env_cube(env, 16, 5), 16, 5, to_device(lut))
        self.lay = HzbLayout(w, h)
        self.bounds = to_device(synth.instances_random(n, 31, center=self.fc.camera_position, box=60.0))
        self.args0 = synth.indirect_args_initial(n)
        self.d_hzb = torch.zeros(self.lay.total, device="cuda")
        self.d_args, self.d_stats = to_device(self.args0), torch.zeros(2, dtype=torch.int32, device="cuda")
        self.d_vis, self.d_cnt = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
        self.consts = hostmath.pack_culling_constants(self.fc.view, self.fc.proj, 0, False, 0, 0, 0, True)
        self._g = {}

    def gbuffer(self, seed):
        from unclerenderer_amd import synth
        from unclerenderer_amd.hotpath import to_device
        if seed not in self._g:
            g = synth.gbuffer_scene(self.fc.view, self.fc.proj, self.fc.camera_position, self.w, self.h, 31 + seed)
            self._g[seed] = (to_device(g.A), to_device(g.B), to_device(g.C), to_device(g.depth), g.hdr)
        return self._g[seed]

    def render(self, frame, seed, flags, ldr, rows=None):
        """One frame; returns the Lighting image it left (device, int16 bits)."""
        torch = _torch()
        from unclerenderer_amd.hotpath import Frame, to_device
        dA, dB, dC, dD, hdr0 = self.gbuffer(seed)
        hdr = to_device(hdr0)
        self.d_args.copy_(to_device(self.args0))
        res = Frame.resources(self.w, self.h, 0, self.h if rows is None else rows, dA, dB, dC, dD, hdr, dD, self.d_hzb, self.lay, self.tables, self.bounds,
                              self.d_args, self.n, 0, self.d_vis, self.d_cnt, self.d_stats, tonemap_band=ldr)
        frame.render(res, self.consts, self.fc.scene, self.fc.sky, flags)
        torch.cuda.synchronize()
        return hdr


@pytest.fixture(scope="module")
def scene(hotpath):
    return _Scene(hotpath)


def _ring(n, h, w):
    torch = _torch()
    return [torch.full((h, w, 4), SENTINEL, dtype=torch.int16, device="cuda") for _ in range(n)]


@pytest.mark.parametrize("fuse", [False, True])
@pytest.mark.parametrize("fif", [3, 1, 2])
def test_frame_sequence_against_the_oracle(hotpath, oracle, scene, fif, fuse):
    """Eleven TAA frames with a different Lighting image each: frame 0 copies, frame k clamps-and-blends frame k - 1's output at
    weight 0.9, rebuilt on the CPU by oracle.temporal_aa from the Lighting image each frame left. taa_next() is checked in front of
    every frame. A frame without the flag, and reset_taa(), each make the next TAA frame a copy with zero jitter again."""
    torch = _torch()
    from unclerenderer_amd import hostmath, lib
    from unclerenderer_amd.hotpath import Frame
    w, h = scene.w, scene.h
    frame = Frame(hotpath, frames_in_flight=fif)
    ring = _ring(fif, h, w)
    frame.set_taa(ring, 0.9)
    ldr = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    base = lib.UR_FRAME_DEFAULT | lib.UR_FRAME_TONEMAP
    taa = base | lib.UR_FRAME_TAA | (lib.UR_FRAME_FUSE_TAA_TONEMAP if fuse else 0)
    names = ["GPU Culling", "Build HZB", "Lighting", "Sky", "TemporalAA", "Tonemap"]
    state = {"prev": None, "prev_write": None, "written": set(), "seed": 0}

    def taa_frame(k_in_run):
        """k_in_run: TAA frames since the history was last dropped."""
        info = frame.taa_next()
        assert info["use_history"] == (k_in_run > 0), (k_in_run, info)
        want_j = hostmath.taa_jitter(k_in_run % 8) if k_in_run > 0 else np.zeros(2, np.float32)
        assert info["jitter"].view(np.uint32).tolist() == want_j.view(np.uint32).tolist(), (k_in_run, info)
        if state["prev_write"] is not None:  # the ring advances with every frame, with or without TAA
            assert info["read_slot"] == state["prev_write"] and info["write_slot"] == (state["prev_write"] + 1) % fif, info
        assert info["read_slot"] == (info["write_slot"] + fif - 1) % fif
        before = [_u16(t).copy() for t in ring]
        ldr.zero_()
        hdr = scene.render(frame, state["seed"], taa, ldr)
        state["seed"] += 1
        cur = _u16(hdr)
        hist = state["prev"] if info["use_history"] else np.zeros_like(cur)
        want = oracle.temporal_aa(cur, hist, 0.9, info["use_history"])
        if not info["use_history"]:
            assert np.array_equal(want, cur)  # a copy
        W = info["write_slot"]
        assert np.array_equal(_u16(ring[W]), want), (k_in_run, W)
        state["written"].add(W)
        for s in range(fif):  # every other slot keeps what it held: the sentinel until its first frame
            if s != W:
                assert np.array_equal(_u16(ring[s]), before[s]), (k_in_run, s)
                if s not in state["written"]:
                    assert (before[s] == SENTINEL).all()
        _assert_tonemap_bytes(_u32(ldr), oracle.tonemap(want, exposure=0.9, gamma=2.2), f"fif={fif} fuse={fuse} frame {k_in_run}")
        rep = frame.report()
        assert [r[0] for r in rep] == names
        assert [r[1] for r in rep] == [fuse and nm == "TemporalAA" for nm in names]
        state["prev"], state["prev_write"] = want, W

    for k in range(11):
        taa_frame(k)
    assert len(state["written"]) == fif

    def plain_frame():
        before = [_u16(t).copy() for t in ring]
        hdr = scene.render(frame, state["seed"], base, ldr)
        state["seed"] += 1
        assert [r[0] for r in frame.report()] == ["GPU Culling", "Build HZB", "Lighting", "Sky", "Tonemap"]
        for s in range(fif):
            assert np.array_equal(_u16(ring[s]), before[s])
        _assert_tonemap_bytes(_u32(ldr), oracle.tonemap(_u16(hdr), exposure=0.9, gamma=2.2), "a frame without TAA")
        state["prev_write"] = (state["prev_write"] + 1) % fif

    # one frame without the flag: the next TAA frame has no history and no jitter, and copies
    plain_frame()
    for k in range(3):
        taa_frame(k)
    # reset_taa likewise
    frame.reset_taa()
    for k in range(3):
        taa_frame(k)
    # a new ring: all invalid again
    frame.set_taa(ring, 0.9)
    taa_frame(0)
    taa_frame(1)
    frame.close()


def test_nothing_else_moved(hotpath, oracle, scene):
    """AutoExposure keeps reading Lighting (luminance[W] is what the same frames give without TAA); with a CAS pass, fused or not,
    the back buffer is ur_cas / ur_tonemap_cas by hand on the expected TAA image; the report lists the pass; a frame without the flag
    writes what a Frame that never had a ring writes."""
    torch = _torch()
    from unclerenderer_amd import lib
    from unclerenderer_amd.hotpath import Frame, to_device
    w, h = scene.w, scene.h
    AE, CAS, FCAS = lib.UR_FRAME_AUTO_EXPOSURE, lib.UR_FRAME_CAS, lib.UR_FRAME_FUSE_TONEMAP_CAS
    TAA, FTAA = lib.UR_FRAME_TAA, lib.UR_FRAME_FUSE_TAA_TONEMAP
    base = lib.UR_FRAME_DEFAULT | lib.UR_FRAME_TONEMAP

    def bits(t):
        return int(_u32(t)[0])

    def make(with_ring):
        f = Frame(hotpath, frames_in_flight=2)
        lum = (torch.full((1,), float("nan"), device="cuda"), torch.full((1,), float("nan"), device="cuda"))
        scratch = torch.zeros((h, w), dtype=torch.int32, device="cuda")
        ring = _ring(2, h, w) if with_ring else None
        if with_ring:
            f.set_taa(ring, 0.9)
        return f, lum, scratch, ring

    fa, lum_a, scr_a, ring = make(True)
    fb, lum_b, scr_b, _ = make(False)
    ldr_a = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    ldr_b = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    full = ["GPU Culling", "Build HZB", "Lighting", "Sky", "TemporalAA", "AutoExposure", "Tonemap", "CAS"]
    prev = None
    combos = [(CAS, "cas"), (CAS | FCAS, "tonemap_cas"), (CAS | FTAA, "cas"), (0, None), (FTAA, None), (CAS, "cas")]
    for k, (extra, how) in enumerate(combos):
        dt = (1 / 60, 1 / 30, 1 / 45)[k % 3]
        fa.set_post(luminance=lum_a, tonemap_scratch=scr_a, delta_time=dt)
        fb.set_post(luminance=lum_b, tonemap_scratch=scr_b, delta_time=dt)
        info = fa.taa_next()
        assert info["use_history"] == (k > 0)
        W = k % 2  # the luminance ping-pong starts at 0 and flips after every AutoExposure frame
        hdr = scene.render(fa, 100 + k, base | AE | TAA | extra, ldr_a)
        # the same frame without TAA on the other Frame: same CAS / fuse flags minus the TAA ones
        scene.render(fb, 100 + k, base | AE | (extra & ~FTAA), ldr_b)
        assert bits(lum_a[W]) == bits(lum_b[W]), k  # AutoExposure read Lighting, not the TAA output
        want = oracle.temporal_aa(_u16(hdr), prev if info["use_history"] else np.zeros_like(_u16(hdr)), 0.9, info["use_history"])
        assert np.array_equal(_u16(ring[info["write_slot"]]), want), k
        prev = want
        # by hand from the expected TAA image with the frame's EV
        d_want = to_device(want)
        by_hand, tmp = torch.zeros_like(ldr_a), torch.zeros_like(ldr_a)
        if how == "tonemap_cas":
            hotpath.tonemap_cas(d_want, by_hand, w, h, exposure=0.9, gamma=2.2, exposure_ev=lum_a[W], sharpness=0.5)
        elif how == "cas":
            hotpath.tonemap(d_want, tmp, w, h, exposure=0.9, gamma=2.2, exposure_ev=lum_a[W])
            hotpath.cas(tmp, by_hand, w, h, sharpness=0.5)
        else:
            hotpath.tonemap(d_want, by_hand, w, h, exposure=0.9, gamma=2.2, exposure_ev=lum_a[W])
        torch.cuda.synchronize()
        assert torch.equal(ldr_a, by_hand), (k, how)
        if k > 0:
            assert not torch.equal(ldr_a, ldr_b), k  # (the blended image is not the Lighting image)
        names = [nm for nm in full if nm != "CAS" or extra & CAS]
        culled = {"TemporalAA"} if extra & FTAA else {"CAS"} if extra & FCAS else set()
        rep = fa.report()
        assert [(r[0], r[1]) for r in rep] == [(nm, nm in culled) for nm in names], (k, rep)
        assert [r[0] for r in fb.report()] == [nm for nm in names if nm != "TemporalAA"]
    # without the flag: the bytes and the report of a Frame that never had a ring (fresh Frames, so that the resource states agree)
    fa.close()
    fb.close()
    fa, lum_a, scr_a, ring = make(True)
    fb, lum_b, scr_b, _ = make(False)
    for k, flags in enumerate((base, base | AE | CAS, base | AE | CAS | FCAS, base | AE)):
        fa.set_post(luminance=lum_a, tonemap_scratch=scr_a, delta_time=1 / 60)
        fb.set_post(luminance=lum_b, tonemap_scratch=scr_b, delta_time=1 / 60)
        ldr_a.zero_()
        ldr_b.zero_()
        ha = scene.render(fa, 200 + k, flags, ldr_a)
        hb = scene.render(fb, 200 + k, flags, ldr_b)
        assert torch.equal(ha, hb) and torch.equal(ldr_a, ldr_b) and torch.equal(scr_a, scr_b), k
        assert bits(lum_a[0]) == bits(lum_b[0]) or (np.isnan(lum_a[0].cpu().numpy()).all() and np.isnan(lum_b[0].cpu().numpy()).all())
        assert bits(lum_a[1]) == bits(lum_b[1]) or (np.isnan(lum_a[1].cpu().numpy()).all() and np.isnan(lum_b[1].cpu().numpy()).all())
        assert fa.report() == fb.report(), k
        assert all((_u16(t) == SENTINEL).all() for t in ring), k
        assert fa.taa_next()["use_history"] is False
    fa.close()
    fb.close()


def test_frame_argument_errors_on_the_device(hotpath, scene):
    """The checks of tests/test_taa_abi.py through the Python face, on a real context: nothing is launched by a refused frame."""
    torch = _torch()
    from unclerenderer_amd import lib
    from unclerenderer_amd.hotpath import Frame
    from unclerenderer_amd.lib import UrError
    w, h = scene.w, scene.h
    frame = Frame(hotpath, frames_in_flight=3)
    ldr = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    base = lib.UR_FRAME_DEFAULT | lib.UR_FRAME_TONEMAP
    with pytest.raises(UrError) as e:
        scene.render(frame, 0, base | lib.UR_FRAME_TAA, ldr)
    assert e.value.code == lib.UR_EINVAL
    with pytest.raises(UrError):
        frame.set_taa(_ring(2, h, w))
    with pytest.raises(UrError):
        frame.taa_next()
    ring = _ring(3, h, w)
    frame.set_taa(ring)
    with pytest.raises(UrError) as e:
        scene.render(frame, 0, base | lib.UR_FRAME_TAA, ldr, rows=h // 2)
    assert e.value.code == lib.UR_EUNSUPPORTED
    with pytest.raises(UrError) as e:
        scene.render(frame, 0, base | lib.UR_FRAME_TAA | lib.UR_FRAME_FUSE_TAA_TONEMAP | lib.UR_FRAME_CAS | lib.UR_FRAME_FUSE_TONEMAP_CAS, ldr)
    assert e.value.code == lib.UR_EINVAL
    assert all((_u16(t) == SENTINEL).all() for t in ring) and int(ldr.abs().max()) == 0
    assert frame.taa_next()["use_history"] is False
    frame.close()
