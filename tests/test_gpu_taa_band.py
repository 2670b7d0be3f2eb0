"""TemporalAA on row bands through the post exchange, on the MI355X, in one process: the standalone calls on virtual bands of a full
frame, and N Frames (rank r of N) with UR_FRAME_TAA_BAND against one unsplit Frame. Everything is held to the unsplit result byte for
byte - the history images, the resolved rows around a band, the LDR band, the EV bits: the band launches run the strip body of the
full-frame launch on the very texels it reads."""
import numpy as np
import pytest

from tests.test_post_band_abi import GPU_SIZES

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A
# quiet NaN, signalling NaN (either sign), +-Inf, negative, 65504
SPECIAL = [0x7E00, 0x7D00, 0xFD00, 0x7C00, 0xFC00, 0xBA00, 0x7BFF]
CASES = [(w, h, n) for w, h, ns in GPU_SIZES for n in ns if h // n >= 2] + [(7, 6, 3)]


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def test_the_cases_are_the_issues():
    assert CASES == [(7, 5, 1), (64, 24, 3), (48, 48, 3), (16, 16, 8), (1920, 1080, 2), (1920, 1080, 4), (1920, 1080, 8), (3840, 2160, 2),
                     (3840, 2160, 3), (3840, 2160, 8), (7680, 4320, 8), (7, 6, 3)]
    assert (16, 16, 8) in CASES and 16 // 8 == 2  # the two-row band: second_row is the last row


def _image(torch, h, w, seed, alpha):
    g = torch.Generator(device="cuda").manual_seed(seed)
    img = (torch.rand((h, w, 4), device="cuda", generator=g) ** 2 * 8).half()
    img[..., 3] = alpha
    return img.view(torch.int16)


def _plant(torch, img, n, salt):
    """Special values in rows row0 - 2 .. row0 + 1 around every band edge, at columns 0, 63, 64 and w - 1 (and their neighbours)."""
    h, w = img.shape[:2]
    band = h // n
    ys, xs, cs, vs, k = [], [], [], [], salt
    for r in range(1, n):
        for y in range(r * band - 2, r * band + 2):
            if not 0 <= y < h:
                continue
            for x in sorted({c for c in (0, 1, 62, 63, 64, 65, w - 2, w - 1) if 0 <= c < w}):
                ys.append(y), xs.append(x), cs.append(k % 3), vs.append(SPECIAL[k % len(SPECIAL)])
                k += 1
    if ys:
        v = torch.tensor(np.array(vs, np.uint16).view(np.int16), device="cuda")
        img[torch.tensor(ys, device="cuda"), torch.tensor(xs, device="cuda"), torch.tensor(cs, device="cuda")] = v


def _u16(t):
    return t.cpu().numpy().view(np.uint16)


@pytest.mark.parametrize("w,h,n", CASES, ids=[f"{w}x{h}/{n}" for w, h, n in CASES])
def test_standalone_calls_equal_the_full_frame(hotpath, oracle, w, h, n):
    torch = _torch()
    from unclerenderer_amd.hotpath import post_record_bytes, taa_record_bytes
    band = h // n
    cur, hist = _image(torch, h, w, 7 * w + h + n, 2.0), _image(torch, h, w, 11 * w + h + n, 1.0)
    _plant(torch, cur, n, 0)
    _plant(torch, hist, n, 3)
    PB, TB = post_record_bytes(w), taa_record_bytes(w)
    ev = torch.tensor([-0.5], device="cuda")
    tkw = dict(exposure=2.0, gamma=2.2, exposure_ev=ev)
    wt = 0.9
    for use in (0, 1):
        # ---- the records, packed over 0xA5: every byte must be written
        post = torch.full((n, PB), 0xA5, dtype=torch.uint8, device="cuda")
        taa = torch.full((n, TB), 0xA5, dtype=torch.uint8, device="cuda")
        for r in range(n):
            r0 = r * band
            hotpath.pack_post_record(cur[r0:r0 + band], post[r], w, h, r0, band)
            hotpath.pack_taa_record(cur[r0:r0 + band], hist[r0:r0 + band] if use else None, use, taa[r], w, h, r0, band)
        torch.cuda.synchronize()
        for r in range(n):
            r0 = r * band
            got = taa[r].cpu().numpy().view(np.uint16).reshape(4, w, 4)
            assert np.array_equal(got[0], _u16(cur[r0 + 1])) and np.array_equal(got[1], _u16(cur[r0 + band - 2])), (use, r)
            if use:
                assert np.array_equal(got[2], _u16(hist[r0])) and np.array_equal(got[3], _u16(hist[r0 + band - 1])), (use, r)
            else:
                assert not got[2:].any(), (use, r)
        trec = taa.view(torch.int16).view(n, 4, w, 4)       # second_row, second_last_row, history_first_row, history_last_row
        prec = post.view(torch.int16).view(n, -1, 4)        # first_row [0, w), last_row [w, 2w), taps
        # ---- the full-frame calls the band forms stand for
        want = torch.full((h, w, 4), SENTINEL, dtype=torch.int16, device="cuda")
        hotpath.temporal_aa(cur, hist, want, wt, use, w, h)
        want_f = torch.full((h, w, 4), SENTINEL, dtype=torch.int16, device="cuda")
        want_ldr = torch.zeros((h, w), dtype=torch.int32, device="cuda")
        hotpath.temporal_aa_tonemap(cur, hist, want_f, want_ldr, wt, use, w, h, **tkw)
        tm_full, want_two, want_fused = (torch.zeros((h, w), dtype=torch.int32, device="cuda") for _ in range(3))
        hotpath.tonemap(want, tm_full, w, h, **tkw)
        hotpath.cas(tm_full, want_two, w, h, sharpness=0.5)
        hotpath.tonemap_cas(want, want_fused, w, h, sharpness=0.5, **tkw)
        torch.cuda.synchronize()
        assert torch.equal(want, want_f)
        if w * h <= 1920 * 1080:  # the yardstick is not only the product's own full-frame path
            ref = oracle.temporal_aa(_u16(cur), _u16(hist), wt, bool(use))
            got = _u16(want)
            nan_r = np.isnan(ref.view(np.float16))
            assert np.array_equal(np.isnan(got.view(np.float16)), nan_r), use
            assert np.array_equal(got[~nan_r], ref[~nan_r]), use  # (a NaN's sign and payload are the hardware's)
        for in_place in (False, True):
            for r in range(n):
                r0 = r * band
                what = (w, h, n, use, in_place, r)
                top, bottom = r == 0, r == n - 1
                above = None if top else prec[r - 1, w:2 * w]
                below = None if bottom else prec[r + 1, :w]
                side = dict(above2=None if top else trec[r - 1, 1], below2=None if bottom else trec[r + 1, 0],
                            hist_above=None if top or not use else trec[r - 1, 3], hist_below=None if bottom or not use else trec[r + 1, 2])
                for fused in (False, True):
                    ra, rb = (torch.full((w, 4), SENTINEL, dtype=torch.int16, device="cuda") for _ in range(2))
                    res = dict(resolved_above=None if top else ra, resolved_below=None if bottom else rb)
                    hb = hist[r0:r0 + band].clone() if use else None
                    out = hb if in_place and use else torch.full((band, w, 4), SENTINEL, dtype=torch.int16, device="cuda")
                    ldr = torch.zeros((band, w), dtype=torch.int32, device="cuda")
                    if fused:
                        hotpath.temporal_aa_tonemap_halo(cur[r0:r0 + band], above, below, hb, out, ldr, wt, use, w, h, r0, band, **side, **res, **tkw)
                    else:
                        hotpath.temporal_aa_halo(cur[r0:r0 + band], above, below, hb, out, wt, use, w, h, r0, band, **side, **res)
                    torch.cuda.synchronize()
                    assert torch.equal(out, want[r0:r0 + band]), (what, fused)
                    assert top or torch.equal(ra, want[r0 - 1]), (what, fused)
                    assert bottom or torch.equal(rb, want[r0 + band]), (what, fused)
                    if fused:
                        assert torch.equal(ldr, want_ldr[r0:r0 + band]), what
                        continue
                    # without the resolved rows: the band's bytes alone (the form of a frame without CAS)
                    out2 = torch.full((band, w, 4), SENTINEL, dtype=torch.int16, device="cuda")
                    hotpath.temporal_aa_halo(cur[r0:r0 + band], above, below, hist[r0:r0 + band] if use else None, out2, wt, use, w, h, r0, band)
                    # Tonemap + CAS behind it, from the resolved rows: fused and not
                    got_fused, got_two = (torch.full((band, w), 0x5A5A5A5A, dtype=torch.int32, device="cuda") for _ in range(2))
                    hotpath.tonemap_cas_halo(out, res["resolved_above"], res["resolved_below"], got_fused, w, h, r0, band, sharpness=0.5, **tkw)
                    hotpath.tonemap(out, ldr, w, band, **tkw)
                    hotpath.cas_halo(ldr, res["resolved_above"], res["resolved_below"], got_two, w, h, r0, band, sharpness=0.5, **tkw)
                    torch.cuda.synchronize()
                    assert torch.equal(out2, want[r0:r0 + band]), what
                    assert torch.equal(got_fused, want_fused[r0:r0 + band]), what
                    assert torch.equal(got_two, want_two[r0:r0 + band]), what


# ---- the frame with virtual ranks ---------------------------------------------------------------------------------------------

FLAG_SETS = ("TAA", "TAA|AE", "TAA|CAS", "TAA|CAS|FUSE", "TAA|FTAA", "TAA|FTAA|CAS")
BASE = ["GPU Culling", "Build HZB", "Lighting", "Sky"]


def _same_next(a, b):
    return (a["read_slot"], a["write_slot"], a["use_history"]) == (b["read_slot"], b["write_slot"], b["use_history"]) and \
        a["jitter"].view(np.uint32).tolist() == b["jitter"].view(np.uint32).tolist()


@pytest.fixture(scope="module")
def inputs(hotpath):
    _torch()
    from tests._post_band_worker import Inputs
    return Inputs(hotpath, 1920, 1080)


@pytest.mark.parametrize("world,fif", [(1, 3), (3, 3), (4, 3), (2, 1), (2, 2)])
def test_frame_bands_equal_the_unsplit_frame(hotpath, inputs, world, fif):
    """Every flag set over frames_in_flight + 3 consecutive frames with a different Lighting image each (the ring wraps, history is
    used), a frame without TAA between the sets: LDR bytes, every ring image, both luminance texels, taa_next() and the report's
    TemporalAA line are the unsplit frame's on every rank, every frame."""
    torch = _torch()
    from tests._post_band_worker import bits
    from tests._taa_band_worker import TaaBandFrame, taa_flags
    inp = inputs
    ref = TaaBandFrame(hotpath, inp, 0, 1, fif)
    bands = [TaaBandFrame(hotpath, inp, r, world, fif) for r in range(world)]
    k = 0

    def frame(spec, dt, next_before=True):
        nonlocal k
        taa = "TAA" in spec
        nxt = ref.frame.taa_next()
        for f in bands:
            assert not next_before or _same_next(f.frame.taa_next(), nxt), (spec, k)
        flags = taa_flags(spec)
        ref.render_k(k, flags, dt, exchange=False)
        exchange = taa or "AE" in spec or "CAS" in spec
        for f in bands:
            f.render_k(k, flags, dt, exchange=True)
            assert [r[0] for r in f.frame.report()] == BASE + (["Post Record"] if exchange else ["Tonemap"]), (spec, k)
        torch.cuda.synchronize()
        if exchange:
            allpost = torch.cat([f.own for f in bands]).view(world, -1)
            alltaa = torch.cat([f.taa_own for f in bands]).view(world, -1)
            for f in bands:
                f.records.copy_(allpost)
                f.taa_records.copy_(alltaa)
            for f in bands:
                f.finish()
        torch.cuda.synchronize()
        what = (spec, k, world, fif)
        assert torch.equal(torch.cat([f.ldr for f in bands]), ref.ldr), what
        for s in range(len(ref.ring)):
            assert torch.equal(torch.cat([f.ring[s] for f in bands]), ref.ring[s]), (what, s)
        for i in (0, 1):
            assert all(bits(f.lum[i]) == bits(ref.lum[i]) for f in bands), (what, i)
        want = [(r[0], r[1]) for r in ref.frame.report()]
        names = BASE + (["TemporalAA"] if taa else []) + (["AutoExposure"] if "AE" in spec else []) + ["Tonemap"] + (["CAS"] if "CAS" in spec else [])
        assert [nm for nm, _ in want] == names, what
        if taa:
            assert ("TemporalAA", "FTAA" in spec) in want
        for f in bands:
            got = [(r[0], r[1]) for r in f.frame.report()]
            assert got == (want[:4] + [("Post Record", False)] + want[4:] if exchange else want), what
        nxt = ref.frame.taa_next()
        assert nxt["use_history"] == taa, what  # the written image is valid after a finished TAA frame, nothing is after any other
        for f in bands:
            assert _same_next(f.frame.taa_next(), nxt), what
        k += 1

    for i, spec in enumerate(FLAG_SETS):
        for j in range(fif + 3):
            frame(spec, (1 / 60, 1 / 30, 1 / 45)[j % 3])
        # a frame without TAA invalidates the ring on every rank, exactly as unsplit (with and without the exchange's passes)
        frame(("CAS", "AE|CAS", "")[i % 3], 1 / 60)
    # a frame that is rendered but never finished hands on nothing either: the next frame's render drops the ring, as the unsplit
    # Frame's does after a frame without TAA (the ring images are compared, so a history that was used would show)
    frame("TAA|CAS", 1 / 60)
    for f in bands:
        f.render_k(k, taa_flags("TAA|CAS"), 1 / 60, exchange=True)
    ref.render_k(k, taa_flags("CAS"), 1 / 60, exchange=False)
    k += 1
    frame("TAA|CAS", 1 / 60, next_before=False)
    frame("TAA|CAS", 1 / 60)
    for f in [ref] + bands:
        f.close()


def test_frame_band_arguments_on_the_device(hotpath, inputs):
    """The frame's checks of tests/test_taa_band_abi.py on a real context: a refused frame launches nothing and leaves nothing pending."""
    torch = _torch()
    from tests._taa_band_worker import TaaBandFrame, taa_flags
    from unclerenderer_amd import lib
    from unclerenderer_amd.hotpath import Frame
    inp = inputs
    f = TaaBandFrame(hotpath, inp, 1, 2)
    base = lib.UR_FRAME_DEFAULT | lib.UR_FRAME_TONEMAP
    # without the new flag: as before
    for flags in (base | lib.UR_FRAME_TAA, base | lib.UR_FRAME_TAA | lib.UR_FRAME_POST_EXCHANGE):
        with pytest.raises(lib.UrError) as e:
            f.frame.render(f.res, f.consts, inp.fc.scene, inp.fc.sky, flags)
        assert e.value.code == lib.UR_EUNSUPPORTED
    # the flag alone, and a frame without TAA records
    with pytest.raises(lib.UrError) as e:
        f.frame.render(f.res, f.consts, inp.fc.scene, inp.fc.sky, base | lib.UR_FRAME_TAA | lib.UR_FRAME_TAA_BAND)
    assert e.value.code == lib.UR_EINVAL
    g = Frame(hotpath, rank=1, world_size=2)
    g.set_post_records(f.own, f.records)
    g.set_taa(f.ring, 0.9)
    with pytest.raises(lib.UrError) as e:
        g.render(f.res, f.consts, inp.fc.scene, inp.fc.sky, base | lib.UR_FRAME_TAA | lib.UR_FRAME_TAA_BAND | lib.UR_FRAME_POST_EXCHANGE)
    assert e.value.code == lib.UR_EINVAL
    with pytest.raises(lib.UrError) as e:
        g.finish_post()
    assert e.value.code == lib.UR_EINVAL
    g.close()
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in f.ring)
    f.render_k(0, taa_flags("TAA"), 1 / 60, exchange=True)  # and a valid one still runs
    f.taa_records[0].copy_(f.taa_own)  # (rank 0's rows are not this test's subject: any bytes)
    f.finish()
    torch.cuda.synchronize()
    assert f.frame.taa_next()["use_history"] is True
    f.close()
