"""AutoExposure and CAS on row bands through the post exchange, on the MI355X, in one process: the standalone calls on virtual bands
of a full frame, and N Frames (rank r of N) with UR_FRAME_POST_EXCHANGE. Everything is held to the unsplit result byte for byte
(EV bits included): the records carry the very texels the full-frame kernels read, and the halo forms share their strip body."""
import numpy as np
import pytest

from tests.test_post_band_abi import GPU_SIZES, ae_taps, slot_rows

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _hdr(h, w, seed):
    """(h, w, 4) uint16 RGBA16F: noise over a gradient, a wide range of luminance."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    base = 0.05 + 2.0 * (x / max(w - 1, 1)) * (y / max(h - 1, 1))
    hdr = np.zeros((h, w, 4), np.float16)
    hdr[..., :3] = (base[..., None] * rng.random((h, w, 3)) ** 2 * 3.0).astype(np.float16)
    hdr[..., 3] = 1.0
    return hdr


SPECIALS = np.array([np.nan, np.inf, -np.inf, -0.75, 65504.0], np.float16)


def _plant_halo_rows(hdr, n):
    """NaN, +-Inf, negative and huge values across the rows on both sides of every band edge."""
    h, w = hdr.shape[:2]
    band = h // n
    for r in range(1, n):
        for y in (r * band - 1, r * band):
            xs = np.arange(y % 3, w, 3)
            hdr[y, xs, (y + xs) % 3] = SPECIALS[(xs + y) % SPECIALS.size]


def _plant_taps(hdr, far_inf: bool):
    """Special values in every tap-slot position: NaN or a negative value in one channel of each tap texel; with far_inf, +-Inf in
    the far row of the taps whose y weight is 0 (only 0 * Inf shows that row, and the result must still be the full frame's)."""
    h, w = hdr.shape[:2]
    x0, x1, y0, y1, _, ay = ae_taps(w, h)
    for i in range(256):
        for k, (x, y) in enumerate(((x0[i], y0[i]), (x1[i], y0[i]), (x0[i], y1[i]), (x1[i], y1[i]))):
            if (i + k) % 5 == 0:
                hdr[y, x, (i + k) % 3] = np.nan
            elif (i + k) % 5 == 1:
                hdr[y, x, (i + k) % 3] = -2.0
            if far_inf and ay[i] == 0 and k >= 2 and y1[i] != y0[i]:
                hdr[y, x, 1] = np.inf if i % 2 else -np.inf


def _records(hotpath, d, w, h, n):
    torch = _torch()
    from unclerenderer_amd.hotpath import post_record_bytes
    band = h // n
    rec = torch.full((n, post_record_bytes(w)), 0xA5, dtype=torch.uint8, device="cuda")  # every byte must be written
    for r in range(n):
        hotpath.pack_post_record(d[r * band:(r + 1) * band], rec[r], w, h, r * band, band)
    torch.cuda.synchronize()
    return rec


def _check_record_layout(rec, hdr_bits, w, h, n):
    """first row, last row, and every tap slot: the texel where the band holds its row, else zero."""
    band = h // n
    rows = slot_rows(w, h)
    x0, x1, y0, y1, _, _ = ae_taps(w, h)
    cols = np.stack([x0, x1, x0, x1], axis=1).reshape(-1)
    for r in range(n):
        got = rec[r].cpu().numpy().view(np.uint16).reshape(-1, 4)
        assert np.array_equal(got[:w], hdr_bits[r * band]) and np.array_equal(got[w:2 * w], hdr_bits[(r + 1) * band - 1])
        mine = (rows >= r * band) & (rows < (r + 1) * band)
        want = np.where(mine[:, None], hdr_bits[rows, cols], 0)
        assert np.array_equal(got[2 * w:], want), r


CASES = [(w, h, n) for w, h, ns in GPU_SIZES for n in ns]


@pytest.mark.parametrize("w,h,n", CASES, ids=[f"{w}x{h}/{n}" for w, h, n in CASES])
def test_standalone_calls_equal_the_full_frame(hotpath, w, h, n):
    torch = _torch()
    from unclerenderer_amd.hotpath import to_device
    band = h // n
    for variant in ("clean", "halo rows", "halo rows and taps"):
        img = _hdr(h, w, 11 + w + h + n)
        if variant != "clean":
            _plant_halo_rows(img, n)
        if variant == "halo rows and taps":
            _plant_taps(img, far_inf=True)
        bits = img.view(np.uint16)
        d = to_device(bits)
        rec = _records(hotpath, d, w, h, n)
        if w * h <= 1920 * 1080:
            _check_record_layout(rec, bits, w, h, n)
        # AutoExposure: the same bits, without and with history (target above and below the previous EV)
        full_ev, band_ev = torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda")
        hotpath.auto_exposure(d, full_ev, w, h)
        hotpath.auto_exposure_records(rec, n, band_ev, w, h)
        torch.cuda.synchronize()
        assert full_ev.cpu().numpy().view(np.uint32)[0] == band_ev.cpu().numpy().view(np.uint32)[0], variant
        assert np.isfinite(full_ev.cpu().numpy()[0])
        for prev in (float(full_ev.cpu()[0]) - 1.25, float(full_ev.cpu()[0]) + 0.5):
            p = torch.tensor([prev], device="cuda")
            hotpath.auto_exposure(d, full_ev, w, h, prev_ev=p, use_history=True, delta_time=1 / 30)
            hotpath.auto_exposure_records(rec, n, band_ev, w, h, prev_ev=p, use_history=True, delta_time=1 / 30)
            torch.cuda.synchronize()
            assert full_ev.cpu().numpy().view(np.uint32)[0] == band_ev.cpu().numpy().view(np.uint32)[0], (variant, prev)
        # Tonemap + CAS on each band from the halo rows of the neighbours' records, fused and not
        ev = torch.tensor([-0.5], device="cuda")
        for kw in (dict(exposure=0.9, sharpness=0.5), dict(exposure=2.0, exposure_ev=ev, sharpness=1.0), dict(exposure=0.9, enable_tonemap=False, sharpness=0.5)):
            tkw = {k: v for k, v in kw.items() if k != "sharpness"}
            want_fused = torch.zeros((h, w), dtype=torch.int32, device="cuda")
            hotpath.tonemap_cas(d, want_fused, w, h, gamma=2.2, **kw)
            ldr = torch.zeros((h, w), dtype=torch.int32, device="cuda")
            want_two = torch.zeros((h, w), dtype=torch.int32, device="cuda")
            hotpath.tonemap(d, ldr, w, h, gamma=2.2, **tkw)
            hotpath.cas(ldr, want_two, w, h, sharpness=kw["sharpness"])
            fused = torch.full((h, w), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
            two = torch.full((h, w), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
            for r in range(n):
                r0 = r * band
                above = rec[r - 1, 8 * w:16 * w] if r > 0 else None
                below = rec[r + 1, :8 * w] if r + 1 < n else None
                hotpath.tonemap_cas_halo(d[r0:r0 + band], above, below, fused[r0:r0 + band], w, h, r0, band, gamma=2.2, **kw)
                ldr_band = torch.zeros((band, w), dtype=torch.int32, device="cuda")
                hotpath.tonemap(d[r0:r0 + band], ldr_band, w, band, gamma=2.2, **tkw)
                hotpath.cas_halo(ldr_band, above, below, two[r0:r0 + band], w, h, r0, band, gamma=2.2, **kw)
            torch.cuda.synchronize()
            assert torch.equal(fused, want_fused), (variant, kw)
            assert torch.equal(two, want_two), (variant, kw)


def test_halo_forms_one_pixel_per_lane(hotpath):
    """The PX = 1 forms at an even width: records at an 8-byte (not 16-byte) offset, bands of 4 rows with a partial strip."""
    torch = _torch()
    from unclerenderer_amd.hotpath import post_record_bytes, to_device
    w, h, n = 96, 12, 3
    img = _hdr(h, w, 5)
    _plant_halo_rows(img, n)
    d = to_device(img.view(np.uint16))
    B = post_record_bytes(w)
    raw = torch.zeros(n * B + 8, dtype=torch.uint8, device="cuda")
    rec = raw[8:].view(n, B)
    band = h // n
    for r in range(n):
        hotpath.pack_post_record(d[r * band:(r + 1) * band], rec[r], w, h, r * band, band)
    want = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    hotpath.tonemap_cas(d, want, w, h, exposure=0.9, gamma=2.2, sharpness=0.5)
    out, two = torch.zeros((h, w), dtype=torch.int32, device="cuda"), torch.zeros((h, w), dtype=torch.int32, device="cuda")
    for r in range(n):
        r0 = r * band
        above, below = (rec[r - 1, 8 * w:16 * w] if r else None), (rec[r + 1, :8 * w] if r + 1 < n else None)
        hotpath.tonemap_cas_halo(d[r0:r0 + band], above, below, out[r0:r0 + band], w, h, r0, band, exposure=0.9, gamma=2.2, sharpness=0.5)
        ldr_band = torch.zeros((band, w), dtype=torch.int32, device="cuda")
        hotpath.tonemap(d[r0:r0 + band], ldr_band, w, band, exposure=0.9, gamma=2.2)
        hotpath.cas_halo(ldr_band, above, below, two[r0:r0 + band], w, h, r0, band, exposure=0.9, gamma=2.2, sharpness=0.5)
    torch.cuda.synchronize()
    assert torch.equal(out, want) and torch.equal(two, want)


# ---- the frame with virtual ranks ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("world", [1, 3, 4])
def test_frame_bands_equal_the_unsplit_frame(hotpath, world):
    torch = _torch()
    from tests._post_band_worker import BandFrame, Inputs, bits, post_flags
    from unclerenderer_amd import lib
    w, h = 1920, 1080
    inp = Inputs(hotpath, w, h)
    ref = BandFrame(hotpath, inp, 0, 1)
    bands = [BandFrame(hotpath, inp, r, world) for r in range(world)]
    base = ["GPU Culling", "Build HZB", "Lighting", "Sky"]
    state = {"W": 0, "T": None}

    def frame(spec, dt, offset=None, reset=False):
        W = state["W"]
        for f in [ref] + bands:
            if reset:
                f.frame.reset_post()
            if offset is not None:
                f.lum[1 - W].fill_(state["T"] + offset)  # the texel the next AutoExposure reads as history (ignored without history)
        ref.render(post_flags(spec), dt, exchange=False)
        for f in bands:
            f.render(post_flags(spec), dt, exchange=True)
            assert [r[0] for r in f.frame.report()] == base + ["Post Record"]
        torch.cuda.synchronize()
        allrec = torch.cat([f.own for f in bands]).view(world, -1)
        for f in bands:
            f.records.copy_(allrec)
        for f in bands:
            f.finish()
        torch.cuda.synchronize()
        got = torch.cat([f.ldr for f in bands])
        assert torch.equal(got, ref.ldr), (spec, dt)
        # the unsplit frame's passes (and culled flags), with "Post Record" between the two halves
        want = [(r[0], r[1]) for r in ref.frame.report()]
        assert [nm for nm, _ in want] == base + (["AutoExposure"] if "AE" in spec else []) + ["Tonemap"] + (["CAS"] if "CAS" in spec else [])
        for f in bands:
            assert [(r[0], r[1]) for r in f.frame.report()] == want[:4] + [("Post Record", False)] + want[4:], spec
        if "AE" in spec:
            want = bits(ref.lum[W])
            assert all(bits(f.lum[W]) == want for f in bands), spec
            if state["T"] is None:
                state["T"] = float(ref.lum[W].cpu()[0])
            state["W"] = 1 - W
        return got

    frame("AE|CAS", 1 / 60)                      # no history
    frame("AE|CAS", 1 / 30, offset=1.5)          # adapts down from above the target
    frame("AE|CAS", 1 / 45, offset=-1.5)         # ... and up from below
    frame("AE|CAS|FUSE", 1 / 45, offset=1.5)     # fused
    frame("AE|CAS", 1 / 45, offset=-1.5, reset=True)  # after reset_post: no history
    frame("CAS|FUSE", 1 / 45)                    # no AutoExposure: the history goes
    frame("AE|CAS|FUSE", 1 / 45, offset=1.5)
    frame("AE|CAS", 1 / 20, offset=-1.5)
    frame("AE", 1 / 20, offset=1.5)              # AutoExposure without CAS: Tonemap alone on the band
    # nothing pending
    for f in bands:
        with pytest.raises(lib.UrError) as e:
            f.finish()
        assert e.value.code == lib.UR_EINVAL
    # the flag without AutoExposure / CAS is ignored: a whole frame renders as before, a band still needs the whole frame only for them
    if world == 1:
        ref.render(0, 1 / 60, exchange=False)
        bands[0].render(0, 1 / 60, exchange=True)
        torch.cuda.synchronize()
        assert torch.equal(bands[0].ldr, ref.ldr) and [r[0] for r in bands[0].frame.report()] == base + ["Tonemap"]
    for f in [ref] + bands:
        f.close()


def test_frame_exchange_arguments(hotpath):
    torch = _torch()
    from tests._post_band_worker import BandFrame, Inputs, post_flags
    from unclerenderer_amd import lib
    from unclerenderer_amd.hotpath import Frame
    w, h = 1920, 1080
    inp = Inputs(hotpath, w, h)
    f = BandFrame(hotpath, inp, 1, 2)
    # a band without the flag: unsupported, as before
    with pytest.raises(lib.UrError) as e:
        f.render(post_flags("AE|CAS"), 1 / 60, exchange=False)
    assert e.value.code == lib.UR_EUNSUPPORTED
    # the flag on a frame without records
    g = Frame(hotpath, rank=1, world_size=2)
    g.set_post(luminance=f.lum, tonemap_scratch=f.scratch)
    with pytest.raises(lib.UrError) as e:
        g.render(f.res, f.consts, inp.fc.scene, inp.fc.sky, lib.UR_FRAME_DEFAULT | lib.UR_FRAME_TONEMAP | lib.UR_FRAME_CAS | lib.UR_FRAME_FUSE_TONEMAP_CAS
                 | lib.UR_FRAME_POST_EXCHANGE)
    assert e.value.code == lib.UR_EINVAL
    with pytest.raises(lib.UrError) as e:
        g.finish_post()
    assert e.value.code == lib.UR_EINVAL
    g.close()
    # rank 0's band on the frame of rank 1: not its equal band
    h0 = BandFrame(hotpath, inp, 0, 2)
    h0.frame.close()
    h0.frame = Frame(hotpath, rank=1, world_size=2)
    h0.frame.set_post_records(h0.own, h0.records)
    with pytest.raises(lib.UrError) as e:
        h0.render(post_flags("AE|CAS|FUSE"), 1 / 60, exchange=True)
    assert e.value.code == lib.UR_EINVAL
    torch.cuda.synchronize()
    for x in (f, h0):
        x.close()
