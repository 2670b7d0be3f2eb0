"""Footprints of the post chain (csrc/tonemap.hip, post.hip, taa.hip): Tonemap, CAS, the fused launch and their halo forms in the
pair, one-pixel and odd-count forms, AutoExposure, TemporalAA on whole frames and bands with every row pointer guarded on its own, and
the two fixed-size records between their neighbours. The rules are those of tests/footprint.py; nothing here judges a value."""
import numpy as np
import pytest

from tests import footprint as F

pytestmark = pytest.mark.gpu


def _hdr(h, w, seed):
    """(h, w, 4) uint16 RGBA16F with a wide range and a few special values."""
    rng = np.random.default_rng(seed)
    img = (rng.random((h, w, 4)) ** 2 * 8).astype(np.float16)
    img[..., 3] = 1.0
    bits = img.view(np.uint16).copy()
    flat = bits.reshape(-1)
    k = rng.integers(0, flat.size, min(16, flat.size))
    flat[k] = np.array([0x7E00, 0x7C00, 0xFC00, 0xBA00, 0x7BFF, 0x0001, 0x8000, 0xFD00], np.uint16)[np.arange(k.size) % 8]
    return bits


def _ldr(h, w, seed):
    return np.random.default_rng(seed).integers(0, 2 ** 32, (h, w), dtype=np.uint32)


# pair form (even counts), odd count, odd width with odd rows, one pixel, one row, full size
POST_SIZES = [(64, 8), (67, 13), (130, 3), (1, 1), (37, 1), (1, 6), (2, 2), (1920, 1080)]
EV = np.array([-0.75], np.float32)


@pytest.mark.parametrize("w,h", POST_SIZES)
def test_tonemap_footprint(hotpath, w, h):
    """ur_tonemap: HDR 8-byte aligned (the one-pixel form) and 512-byte aligned (the pair form), with and without the EV texel."""
    hdr = _hdr(h, w, 1)
    for align in (512, 8):
        for ev in (None, EV):
            def call(b):
                hotpath.tonemap(b["hdr"], b["out"], w, h, exposure=0.9, gamma=2.2, exposure_ev=b["ev"])
            F.run_rules(call, {"hdr": hdr, "ev": ev}, {"out": _ldr(h, w, 2)}, aligns={"hdr": align, "ev": 4},
                        what=f"tonemap {w}x{h} align {align}")
    # a band of the image: w x rows is all the call knows
    if h >= 3:
        F.run_rules(lambda b: hotpath.tonemap(b["hdr"], b["out"], w, h - 2, exposure=2.0, gamma=2.2), {"hdr": hdr[1:h - 1]},
                    {"out": _ldr(h - 2, w, 3)}, what=f"tonemap band {w}x{h}")


@pytest.mark.parametrize("w,h", POST_SIZES)
def test_cas_footprint(hotpath, w, h):
    """ur_cas (LDR input 4-byte aligned: the one-pixel form) and ur_tonemap_cas (HDR 8-byte aligned), whole frames and bands."""
    ldr, hdr = _ldr(h, w, 4), _hdr(h, w, 5)
    bands = sorted({(0, h), (0, 1), (h - 1, 1), (h // 2, max(1, h // 3))})
    for row0, rows in bands:
        if row0 + rows > h:
            continue
        for align in (512, 4):
            F.run_rules(lambda b: hotpath.cas(b["ldr"], b["out"], w, h, row0=row0, rows=rows, sharpness=1.0), {"ldr": ldr},
                        {"out": _ldr(rows, w, 6)}, aligns={"ldr": align}, what=f"cas {w}x{h} rows {row0}+{rows} align {align}")
        for align in (512, 8):
            F.run_rules(lambda b: hotpath.tonemap_cas(b["hdr"], b["out"], w, h, row0=row0, rows=rows, exposure=2.0, gamma=2.2, sharpness=0.5,
                                                      exposure_ev=b["ev"]), {"hdr": hdr, "ev": EV}, {"out": _ldr(rows, w, 7)},
                        aligns={"hdr": align, "ev": 4}, what=f"tonemap_cas {w}x{h} rows {row0}+{rows} align {align}")


@pytest.mark.parametrize("w,h,row0,rows", [(64, 24, 8, 8), (67, 13, 0, 5), (67, 13, 8, 5), (130, 9, 3, 3), (1, 3, 1, 1), (16, 16, 14, 2),
                                           (1920, 1080, 270, 270)])
def test_cas_halo_footprint(hotpath, w, h, row0, rows):
    """ur_tonemap_cas_halo and ur_cas_halo: the band and each halo row on its own allocation."""
    hdr, ldr = _hdr(h, w, 8), _ldr(h, w, 9)
    top, bottom = row0 == 0, row0 + rows == h
    ins = {"above": None if top else hdr[row0 - 1], "below": None if bottom else hdr[row0 + rows], "ev": EV}
    rb = {"above": w * 8, "below": w * 8}
    for align in (512, 8):
        al = {"band": align, "above": align, "below": align, "ev": 4}
        F.run_rules(lambda b: hotpath.tonemap_cas_halo(b["band"], b["above"], b["below"], b["out"], w, h, row0, rows, exposure=2.0, gamma=2.2,
                                                       exposure_ev=b["ev"], sharpness=0.5),
                    dict(ins, band=hdr[row0:row0 + rows]), {"out": _ldr(rows, w, 10)}, aligns=al, row_bytes=rb,
                    what=f"tonemap_cas_halo {w}x{h} {row0}+{rows} align {align}")
    for align in (512, 4):
        al = {"band": align, "above": 8 if align == 4 else 512, "below": 8 if align == 4 else 512, "ev": 4}
        F.run_rules(lambda b: hotpath.cas_halo(b["band"], b["above"], b["below"], b["out"], w, h, row0, rows, exposure=2.0, gamma=2.2,
                                               exposure_ev=b["ev"], sharpness=1.0),
                    dict(ins, band=ldr[row0:row0 + rows]), {"out": _ldr(rows, w, 11)}, aligns=al, row_bytes=rb,
                    what=f"cas_halo {w}x{h} {row0}+{rows} align {align}")


@pytest.mark.parametrize("h,w", [(1080, 1920), (2160, 3840), (131, 257), (9, 17)])  # as tests/test_gpu_post.py, SIZES_AE
def test_auto_exposure_footprint(hotpath, h, w):
    """ur_auto_exposure and ur_auto_exposure_records: each luminance float between guards of its own."""
    from unclerenderer_amd.hotpath import post_record_bytes
    hdr = _hdr(h, w, 12)
    prev, out0 = np.array([1.25], np.float32), np.array([np.nan], np.float32)
    kw = dict(use_history=True, delta_time=1 / 30)
    F.run_rules(lambda b: hotpath.auto_exposure(b["hdr"], b["out"], w, h), {"hdr": hdr}, {"out": out0}, aligns={"out": 4},
                what=f"auto_exposure {w}x{h}")
    for align in (512, 8):
        F.run_rules(lambda b: hotpath.auto_exposure(b["hdr"], b["out"], w, h, prev_ev=b["prev"], **kw), {"hdr": hdr, "prev": prev}, {"out": out0},
                    aligns={"hdr": align, "prev": 4, "out": 4}, what=f"auto_exposure history {w}x{h} align {align}")
    # prev may be out: one float read and written
    F.run_rules(lambda b: hotpath.auto_exposure(b["hdr"], b["lum"], w, h, prev_ev=b["lum"], **kw), {"hdr": hdr}, {"lum": prev}, aligns={"lum": 4},
                what=f"auto_exposure in place {w}x{h}")
    n = next(k for k in (3, 2, 1) if h % k == 0)
    band = h // n
    PB = post_record_bytes(w)

    def pack(b):
        for r in range(n):
            hotpath.pack_post_record(b["hdr"][r * band:(r + 1) * band], b["records"][r], w, h, r * band, band)
        hotpath.auto_exposure_records(b["records"], n, b["out"], w, h, prev_ev=b["prev"], **kw)

    base = F.run_rules(pack, {"hdr": hdr, "prev": prev}, {"records": np.full((n, PB), 0xA5, np.uint8), "out": out0},
                       aligns={"prev": 4, "out": 4}, what=f"auto_exposure_records {w}x{h}/{n}")
    # the gathered records as an input of their own
    F.run_rules(lambda b: hotpath.auto_exposure_records(b["records"], n, b["out"], w, h, prev_ev=b["prev"], **kw),
                {"records": base["records"], "prev": prev}, {"out": out0}, aligns={"records": 16, "prev": 4, "out": 4},
                what=f"auto_exposure_records read {w}x{h}/{n}")


TAA_SIZES = [(64, 8), (67, 13), (130, 3), (513, 17), (1, 1), (2251, 4001)]


@pytest.mark.parametrize("w,h", TAA_SIZES)
def test_temporal_aa_footprint(hotpath, w, h):
    """ur_temporal_aa and ur_temporal_aa_tonemap: whole frames, bands off the 8-row grid, a first, a last and a two-row band, in place
    and not, 8-byte aligned images."""
    cur, hist = _hdr(h, w, 13), _hdr(h, w, 14)
    big = w * h > 1_000_000
    bands = [(0, h)] if big else sorted({(0, h), (0, min(h, 3)), (max(h - 5, 0), min(h, 5)), (min(3, h - 1), min(2, h - min(3, h - 1))),
                                         (h // 2, max(1, min(11, h - h // 2)))})
    for row0, rows in bands:
        for use in (0, 1):
            for align in ((512,) if big else (512, 8)):
                al = {"cur": align, "hist": align, "out": align, "ev": 4}
                what = f"{w}x{h} rows {row0}+{rows} use {use} align {align}"
                F.run_rules(lambda b: hotpath.temporal_aa(b["cur"], b["hist"], b["out"], 0.9, use, w, h, row0, rows),
                            {"cur": cur, "hist": hist[row0:row0 + rows]}, {"out": _hdr(rows, w, 15)}, aligns=al, what="temporal_aa " + what)
                if use and align == 512:  # a ring of one image: the history is the output
                    F.run_rules(lambda b: hotpath.temporal_aa(b["cur"], b["hist"], b["hist"], 0.9, 1, w, h, row0, rows),
                                {"cur": cur}, {"hist": hist[row0:row0 + rows]}, what="temporal_aa in place " + what)
                if big and use == 0:
                    continue
                F.run_rules(lambda b: hotpath.temporal_aa_tonemap(b["cur"], b["hist"], b["out"], b["ldr"], 0.9, use, w, h, row0, rows, exposure=2.0,
                                                                  gamma=2.2, exposure_ev=b["ev"]),
                            {"cur": cur, "hist": hist[row0:row0 + rows], "ev": EV}, {"out": _hdr(rows, w, 16), "ldr": _ldr(rows, w, 17)},
                            aligns=al, what="temporal_aa_tonemap " + what)


@pytest.mark.parametrize("w,h,row0,rows", [(64, 24, 8, 8), (67, 13, 0, 5), (67, 13, 8, 5), (67, 13, 3, 7), (130, 9, 3, 2), (16, 16, 14, 2),
                                           (513, 17, 5, 9), (1920, 1080, 270, 270)])
def test_temporal_aa_halo_footprint(hotpath, w, h, row0, rows):
    """ur_temporal_aa_halo and ur_temporal_aa_tonemap_halo: the band, the two current halo rows, the two second rows, the two history
    rows and the two resolved rows each on an allocation of its own; with and without the resolved rows, in place and not."""
    cur, hist = _hdr(h, w, 18), _hdr(h, w, 19)
    top, bottom = row0 == 0, row0 + rows == h
    rowb = w * 8
    for use in (0, 1):
        for resolve in (False, True):
            ins = {"band": cur[row0:row0 + rows], "above": None if top else cur[row0 - 1], "below": None if bottom else cur[row0 + rows],
                   "hist": hist[row0:row0 + rows] if use else None, "ev": EV,
                   "above2": cur[max(row0 - 2, 0)] if resolve and not top else None,
                   "below2": cur[min(row0 + rows + 1, h - 1)] if resolve and not bottom else None,
                   "hist_above": hist[row0 - 1] if resolve and use and not top else None,
                   "hist_below": hist[row0 + rows] if resolve and use and not bottom else None}
            outs = {"out": _hdr(rows, w, 20), "ldr": _ldr(rows, w, 21),
                    "res_above": _hdr(1, w, 22)[0] if resolve and not top else None, "res_below": _hdr(1, w, 23)[0] if resolve and not bottom else None}
            rb = {k: rowb for k in ("above", "below", "above2", "below2", "hist_above", "hist_below", "res_above", "res_below")}
            for align in (512, 8):
                al = {k: align for k in list(ins) + list(outs)}
                al["ev"] = 4
                al["ldr"] = 512
                what = f"{w}x{h} rows {row0}+{rows} use {use} resolve {resolve} align {align}"
                side = lambda b: dict(above2=b["above2"], hist_above=b["hist_above"], below2=b["below2"], hist_below=b["hist_below"],  # noqa: E731
                                      resolved_above=b["res_above"], resolved_below=b["res_below"])
                plain_outs = {k: v for k, v in outs.items() if k != "ldr"}
                F.run_rules(lambda b: hotpath.temporal_aa_halo(b["band"], b["above"], b["below"], b["hist"], b["out"], 0.9, use, w, h, row0, rows, **side(b)),
                            ins, plain_outs, aligns=al, row_bytes=rb, what="temporal_aa_halo " + what)
                F.run_rules(lambda b: hotpath.temporal_aa_tonemap_halo(b["band"], b["above"], b["below"], b["hist"], b["out"], b["ldr"], 0.9, use, w, h,
                                                                       row0, rows, exposure=2.0, gamma=2.2, exposure_ev=b["ev"], **side(b)),
                            ins, outs, aligns=al, row_bytes=rb, what="temporal_aa_tonemap_halo " + what)
            if use and resolve:  # the history read and written in place
                ins2 = {k: v for k, v in ins.items() if k != "hist"}
                outs2 = {"hist": hist[row0:row0 + rows], "res_above": outs["res_above"], "res_below": outs["res_below"]}
                F.run_rules(lambda b: hotpath.temporal_aa_halo(b["band"], b["above"], b["below"], b["hist"], b["hist"], 0.9, 1, w, h, row0, rows,
                                                               above2=b["above2"], hist_above=b["hist_above"], below2=b["below2"],
                                                               hist_below=b["hist_below"], resolved_above=b["res_above"], resolved_below=b["res_below"]),
                            ins2, outs2, row_bytes=rb, what=f"temporal_aa_halo in place {w}x{h} rows {row0}+{rows}")


@pytest.mark.parametrize("w,h,row0,rows", [(64, 24, 8, 8), (67, 13, 0, 13), (67, 12, 4, 4), (7, 6, 2, 2), (1, 1, 0, 1), (1920, 1080, 540, 270),
                                           (3840, 2160, 1080, 270)])
def test_pack_records_footprint(hotpath, w, h, row0, rows):
    """ur_pack_post_record and ur_pack_taa_record into the middle slot of three adjacent slots of exactly ur_post_record_bytes(w) /
    ur_taa_record_bytes(w): the outer slots keep their fill, and so do the guards around the three."""
    from unclerenderer_amd.hotpath import post_record_bytes, taa_record_bytes
    cur, hist = _hdr(h, w, 24), _hdr(h, w, 25)
    PB, TB = post_record_bytes(w), taa_record_bytes(w)
    assert PB == (2 * w + 1024) * 8 and TB == 32 * w
    rng = np.random.default_rng(26)
    outer = lambda r: {"slots": np.arange(3)[:, None].repeat(r["slots"].shape[1], 1) != 1}  # noqa: E731
    for align in (512, 8):
        F.run_rules(lambda b: hotpath.pack_post_record(b["band"], b["slots"][1], w, h, row0, rows), {"band": cur[row0:row0 + rows]},
                    {"slots": rng.integers(0, 256, (3, PB), dtype=np.uint8)}, aligns={"band": align, "slots": align}, untouched=outer,
                    what=f"pack_post_record {w}x{h} {row0}+{rows} align {align}")
        for use in (0, 1):
            F.run_rules(lambda b: hotpath.pack_taa_record(b["band"], b["hist"], use, b["slots"][1], w, h, row0, rows),
                        {"band": cur[row0:row0 + rows], "hist": hist[row0:row0 + rows] if use else None},
                        {"slots": rng.integers(0, 256, (3, TB), dtype=np.uint8)}, aligns={"band": align, "hist": align, "slots": align},
                        untouched=outer, what=f"pack_taa_record {w}x{h} {row0}+{rows} use {use} align {align}")


def test_detector_tonemap_one_row_too_many(hotpath):
    """The write rule bites: ur_tonemap told rows + 1 on a payload of `rows` rows writes exactly one row behind it - into the guard,
    not out of the allocation (the input is a full rows + 1 image, so nothing is read out of bounds either)."""
    import torch
    w, rows = 200, 9
    hdr = F.plain(_hdr(rows + 1, w, 27), "cuda")
    out = F.guarded(_ldr(rows, w, 28), "cuda", ("hash", 1))
    assert F.check(out).ok
    hotpath.tonemap(hdr, out, w, rows + 1, exposure=1.0, gamma=2.2)
    torch.cuda.synchronize()
    r = F.check(out)
    print(r)
    assert not r.ok and r.rows_touched() == [rows], str(r)
    assert r.first >= rows * w * 4 and r.last < (rows + 1) * w * 4 and r.where(r.first)[0] == rows
    # a position-dependent fill: nearly every byte of the row differs from what the kernel wrote (alpha alone could hide under 0xFF)
    assert r.offsets.size > 0.97 * w * 4
