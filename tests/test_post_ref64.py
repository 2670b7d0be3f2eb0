"""The float64 restatement of the post chain (tests/post_ref64.py) on the CPU: hand-derived known answers, the fp32 oracle and
tests/post_ref.py held to its rules, and planted errors that the old tolerance lets through but the rules do not."""
import math

import numpy as np
import pytest

from tests import post_ref, post_ref64 as P

F32 = np.float32


def _c(v):
    return float(F32(v))


def _px(*rgb):
    """One RGBA16F pixel, (1, 4) uint16 bits; alpha 1."""
    a = np.array([list(rgb) + [1.0]], np.float64).astype(np.float16)
    return a.view(np.uint16)


def _bits(*vals):
    return np.array([vals], np.uint16)


def hdr_bits(h, w, seed, scale=1.0):
    """tests/test_gpu_post.py:_hdr_bits - a smooth gradient times noise."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    base = 0.05 + 2.0 * (x / max(w - 1, 1)) * (y / max(h - 1, 1))
    hdr = np.zeros((h, w, 4), np.float16)
    hdr[..., :3] = np.minimum(base[..., None] * (rng.random((h, w, 3)) ** 2 * 3.0) * scale, 60000).astype(np.float16)
    hdr[..., 3] = 1.0
    return hdr.view(np.uint16)


def cube_bits(h, w, seed):
    """rng ** 3 * 6, as tests/test_gpu_parity.py:test_tonemap_parity."""
    rng = np.random.default_rng(seed)
    hdr = np.zeros((h, w, 4), np.float16)
    hdr[..., :3] = (rng.random((h, w, 3)) ** 3 * 6.0).astype(np.float16)
    hdr[..., 3] = 2.0
    return hdr.view(np.uint16)


def ldr(h, w, seed):
    """tests/test_gpu_post.py:_ldr - flat-ish and noisy regions."""
    rng = np.random.default_rng(seed)
    b = rng.integers(0, 256, (h, w, 3)).astype(np.uint32)
    b[: h // 2] = (b[: h // 2] // 32) * 32 + 16
    return (b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16) | np.uint32(0xFF000000)).astype(np.uint32)


# ---- known answers -------------------------------------------------------------------------------------------------------
START = float(F32(0.8) - F32(0.04))
D = 1.0 - START


def _neutral(r, g, b, desat=_c(0.15)):
    """PBRNeutralToneMapping of one float64 colour, scalar, straight from Tonemap.hlsl:34-55."""
    x = min(r, g, b)
    off = x - _c(6.25) * x * x if x < _c(0.08) else _c(0.04)
    r, g, b = r - off, g - off, b - off
    peak = max(r, g, b)
    if peak < START:
        return r, g, b
    new_peak = 1.0 - D * D / (peak + D - START)
    s = new_peak / max(peak, _c(1e-4))
    gm = 1.0 - 1.0 / (desat * (peak - new_peak) + 1.0)
    return tuple(c * s + gm * (new_peak - c * s) for c in (r, g, b))


def test_tonemap_known_answers():
    e = P.inv_gamma(2.2)
    assert e == float(F32(1) / F32(2.2))
    # x just below / at 0.08: the quadratic offset, then the constant one (fp16 0.08 is 0.0800170898..., above the fp32 0.08)
    for x in (float(np.float16(0.0799)), float(np.float16(0.08))):
        assert (x < _c(0.08)) == (x < 0.08)
        lin, v, comp = P.tonemap64(_px(x, 0.5, 0.25))
        off = x - _c(6.25) * x * x if x < _c(0.08) else _c(0.04)
        assert not comp[0] and np.array_equal(lin[0], np.array([x, 0.5, 0.25]) - off)
        assert np.allclose(v[0], np.power(np.array([x, 0.5, 0.25]) - off, e) * 255, rtol=1e-15)
    # peak on startCompression: the branch is continuous there (newPeak = peak, s = 1, g = 0)
    lin, _, comp = P.tonemap64(_px(1.0, 1.0, 1.0), exposure=START + _c(0.04))
    peak = _c(START + _c(0.04)) - _c(0.04)
    assert comp[0] == (not peak < START)
    assert np.allclose(lin[0], peak, rtol=0, atol=1e-7)
    # a grey of 1: x = 1, offset 0.04, peak 0.96 -> compressed
    lin, v, comp = P.tonemap64(_px(1.0, 1.0, 1.0))
    want = _neutral(1.0, 1.0, 1.0)
    assert comp[0] and np.allclose(lin[0], want, rtol=1e-15)
    # EnableTonemap off: exposure and gamma only
    lin, v, _ = P.tonemap64(_px(0.25, 2.0, 0.0), exposure=0.9, enable_tonemap=False)
    assert np.array_equal(lin[0], np.array([0.25, 2.0, 0.0]) * _c(0.9))
    assert P.tonemap_bytes(v)[0].tolist() == [round(255 * (0.25 * _c(0.9)) ** e + 1e-9), 255, 0]
    # exposure_ev multiplies by 2^EV exactly
    lin, _, _ = P.tonemap64(_px(0.25, 0.5, 0.125), exposure=2.0, exposure_ev=-1.5, enable_tonemap=False)
    assert np.allclose(lin[0], np.array([0.25, 0.5, 0.125]) * 2.0 * 2.0 ** float(F32(-1.5)), rtol=1e-15)


def test_tonemap_non_finite_and_edge_pixels(oracle):
    """The reference's formula on non-finite HDR, derived by hand (and what the oracle gives):
    (+Inf, 0, 0): x = 0, offset 0, peak = Inf, newPeak = 1, s = 0 -> R = Inf * 0 = NaN, g = 1 - 1/Inf = 1 -> G = B = lerp(0, 1, 1)
    = 1: R saturates to 0, cyan. (Inf, Inf, Inf): offset 0.04, peak Inf, every channel Inf * 0 = NaN -> black. (NaN, 0, 0): the
    min and max ignore the NaN, peak 0, no compression, saturate(NaN) = 0 -> black. (-1, 0.5, 0.5): offset -1 - 6.25 = -7.25,
    colour (6.25, 7.75, 7.75), newPeak = 1 - 0.0576 / 7.23, s = newPeak / 7.75, g = 1 - 1 / (0.15 * (7.75 - newPeak) + 1)
    -> (0.89668, 0.99203, 0.99203) -> (243, 254, 254): near white. 65504 red: peak 65504, R = newPeak ~ 1, g ~ 0.9999 -> white.
    -0: black. (2^-24, 2^-20, 6.1e-5): offset ~ 2^-24, B = 6.1e-5^(1/2.2) * 255 = 3.1 -> 3, G = 0.47 -> 0."""
    inf, nan = float("inf"), float("nan")
    cases = [((inf, 0, 0), (0, 255, 255)), ((inf, inf, inf), (0, 0, 0)), ((nan, 0, 0), (0, 0, 0)), ((-1.0, 0.5, 0.5), (243, 254, 254)),
             ((65504.0, 0, 0), (255, 255, 255)), ((-0.0, -0.0, -0.0), (0, 0, 0)), ((2.0 ** -24, 2.0 ** -20, 6.1e-5), (0, 0, 3)),
             ((-inf, 0.5, 0.5), (0, 0, 0)), ((0, nan, 0.5), None), ((-65504.0, 0, 0), None)]
    for rgb, want in cases:
        bits = _px(*rgb)
        lin, v, comp = P.tonemap64(bits)
        dec, byte = P.tonemap_decide(lin, comp, 2.2)
        ref = P.channels(oracle.tonemap(bits))[0]
        assert dec[0].all(), rgb
        assert byte[0].tolist() == ref.tolist(), (rgb, byte[0], ref)
        if want is not None:
            assert byte[0].tolist() == list(want), (rgb, byte[0])
    # the exact value of the near-white pixel, by hand
    lin, _, _ = P.tonemap64(_px(-1.0, 0.5, 0.5))
    assert np.allclose(lin[0], _neutral(-1.0, 0.5, 0.5), rtol=1e-15)
    np_ = 1.0 - D * D / (7.75 + D - START)
    assert math.isclose(lin[0, 1], np_, rel_tol=1e-15)


def test_cas_known_answers():
    # a flat image is a fixed point: sharpL = (4 L w + L) / (4 w + 1) = L, out = C
    for v in (0, 1, 77, 254, 255):
        img = np.full((5, 7), v * 0x010101 | 0xFF000000, np.uint32)
        x = P.cas64(img, 1.0)
        assert np.allclose(x, v / 255.0, rtol=0, atol=1e-15), v
        dec, byte = P.cas_decide(x)
        assert dec.all() and (byte == v).all()
    # a grey step from 64 to 192 (columns 0-2 | 3-5): the pixel right of the edge, by hand
    img = np.full((3, 6), 64 * 0x010101 | 0xFF000000, np.uint32)
    img[:, 3:] = 192 * 0x010101 | 0xFF000000
    lo, hi, eps, lum = 64 / 255, 192 / 255, _c(1e-4), _c(0.2126) + _c(0.7152) + _c(0.0722)
    amp = 1.0 / math.sqrt(min(lo, 2.0 - hi) / (hi + eps) + eps)
    w = -_c(0.2) / (amp * lum)
    sharp_l = min(max(((3 * hi + lo) * lum * w + hi * lum) / (4 * w + 1), 0.0), 1.0)
    for s in (0.5, 1.0):
        want = hi + _c(s) * ((hi - hi * lum + sharp_l) - hi)
        x = P.cas64(img, s)
        assert np.allclose(x[1, 3], want, rtol=1e-14), (x[1, 3], want)
        assert want > hi  # the bright side of the edge brightens
        # and the dark side darkens, symmetric: its left neighbour is dark, right is bright
        assert (x[1, 2] < lo).all()
    assert np.allclose(P.cas64(img, 0.0), P.channels(img) / 255.0, rtol=0, atol=0)


def test_temporal_aa_known_answers():
    h16 = lambda a: np.asarray(a, np.float16).view(np.uint16)
    cur = np.zeros((3, 3, 4), np.float16)
    cur[..., :3] = 0.5
    cur[1, 1, :3] = [1.0, 0.25, 0.5]
    cur[..., 3] = 2.0
    hist = np.zeros((3, 3, 4), np.float16)
    hist[..., :3] = [4.0, 0.0, 0.375]   # red above the box, green below it, blue inside (box b at (0,0): [0.5, 0.5])
    hist[1, 1, 2] = 0.5
    out = P.temporal_aa64(h16(cur), h16(hist), 0.9)
    w = _c(0.9)
    # centre: box r [0.5, 1], g [0.25, 0.5], b [0.5, 0.5] -> history (1, 0.25, 0.5) = current
    assert out[1, 1].tolist() == [1.0, 0.25, 0.5, 2.0]
    # corner (0, 0): the same box; history clamps to (1, 0.25, 0.5) against a current of 0.5
    assert np.allclose(out[0, 0], [0.5 + w * 0.5, 0.5 + w * (0.25 - 0.5), 0.5, 2.0], rtol=1e-15)
    # inside the box: a history of 0.75 in red stays 0.75
    hist2 = hist.copy()
    hist2[0, 0, 0] = 0.75
    assert math.isclose(P.temporal_aa64(h16(cur), h16(hist2), 0.9)[0, 0, 0], 0.5 + w * 0.25, rel_tol=1e-15)
    # NaN weight -> saturate(NaN) = 0: the current frame; above 1 -> 1: the clamped history
    assert np.array_equal(P.temporal_aa64(h16(cur), h16(hist), float("nan"))[..., :3], cur[..., :3].astype(np.float64))
    assert np.allclose(P.temporal_aa64(h16(cur), h16(hist), 7.0)[0, 0, :3], [1.0, 0.25, 0.5])
    # a NaN (quiet or signalling pattern) in the neighbourhood is ignored by min / max; a NaN history clamps to min
    for nb in (0x7E00, 0x7D00, 0xFD00):
        c2 = h16(cur).copy()
        c2[2, 2, :3] = nb
        assert np.array_equal(P.temporal_aa64(c2, h16(hist), 0.9)[1, 1], out[1, 1]), hex(nb)
    h2 = h16(hist).copy()
    h2[0, 0, :3] = 0x7D00
    assert np.allclose(P.temporal_aa64(h16(cur), h2, 0.9)[0, 0, :3], [0.5, 0.5 + w * (0.25 - 0.5), 0.5])


def test_auto_exposure_known_answers():
    key_ev, min_ev, max_ev = math.log2(_c(0.3)), math.log2(_c(0.1)), math.log2(_c(5.0))
    lum = _c(0.2126) + _c(0.7152) + _c(0.0722)
    grey = lambda h, w, v: np.tile(_px(v, v, v).reshape(1, 1, 4), (h, w, 1))
    # a constant frame, and 1x1 (every tap clamps onto the one texel)
    for h, w in ((9, 17), (1, 1), (1, 37), (37, 1)):
        ev = P.ae_log_average64(grey(h, w, 0.25))
        assert math.isclose(ev, math.log2(0.25 * lum), rel_tol=1e-14), (h, w)
        assert math.isclose(P.ae_adapt64(ev), min(max(key_ev - ev, min_ev), max_ev), rel_tol=1e-14)
    # 1 x 16: the taps land on texel centres (t = g), each column once per row of taps
    row = np.array([2.0 ** (k - 8) for k in range(16)])
    img = np.stack([np.concatenate([_px(v, v, v) for v in row])], 0)
    assert math.isclose(P.ae_log_average64(img), float(np.mean(np.log2(np.maximum(row * lum, _c(1e-4))))), rel_tol=1e-14)
    # 1 x 32: t = 2g + 0.5, halfway between texels 2g and 2g + 1
    row = np.arange(1, 33) / 8.0
    img = np.stack([np.concatenate([_px(v, v, v) for v in row])], 0)
    want = float(np.mean(np.log2((row[0::2] + row[1::2]) / 2 * lum)))
    assert math.isclose(P.ae_log_average64(img), want, rel_tol=1e-14)
    # an Inf texel where a tap's last corner lands with positive weights (32 x 32: tap (0, 0) blends texels 0 and 1 by 0.5):
    # log2(Inf) makes the average Inf and the target clamps to minEv
    img = grey(32, 32, 0.25)
    img[1, 1, :3] = 0x7C00
    assert P.ae_log_average64(img) == math.inf and P.ae_adapt64(P.ae_log_average64(img)) == min_ev
    # an all-NaN frame: max(NaN, 0) = 0, luminance floored at 1e-4
    nan = np.full((8, 8, 4), 0x7E00, np.uint16)
    ev = P.ae_log_average64(nan)
    assert math.isclose(ev, math.log2(_c(1e-4)), rel_tol=1e-15)
    assert math.isclose(P.ae_adapt64(ev, ev_max=1e6), key_ev - math.log2(_c(1e-4)), rel_tol=1e-15)
    # history: alpha = 1 - exp(-dt * speed), speed by direction
    for prev, speed in ((-3.0, 3.0), (3.0, 1.0)):
        t = P.ae_adapt64(0.0)
        a = 1.0 - math.exp(-_c(1 / 30) * speed)
        assert math.isclose(P.ae_adapt64(0.0, prev=prev, use_history=True, delta_time=1 / 30), prev + a * (t - prev), rel_tol=1e-14)


# ---- the fp32 oracle and post_ref meet the rules ---------------------------------------------------------------------------
TM_FIXTURES = {"gradient": lambda: hdr_bits(384, 512, 3), "cube": lambda: cube_bits(384, 512, 4)}
TM_PARAMS = [dict(exposure=0.3), dict(exposure=0.9), dict(exposure=1.0), dict(exposure=2.0), dict(exposure=1.0, gamma=1.0),
             dict(exposure=0.9, gamma=1e-4), dict(exposure=0.9, enable_tonemap=False), dict(exposure=2.0, exposure_ev=-1.5)]


def _tm_rule(bits, **kw):
    lin, v, comp = P.tonemap64(bits, **kw)
    dec, want = P.tonemap_decide(lin, comp, kw.get("gamma", 2.2))
    return dec, want, P.tonemap_bytes(v)


@pytest.mark.parametrize("fx", list(TM_FIXTURES))
def test_oracle_tonemap_meets_the_byte_rule(oracle, fx, record_property):
    bits = TM_FIXTURES[fx]()
    for kw in TM_PARAMS:
        dec, want, exact = _tm_rule(bits, **kw)
        r = P.byte_check(P.channels(oracle.tonemap(bits, **kw)), dec, want, exact)
        name = ",".join(f"{k}={v}" for k, v in kw.items())
        record_property(f"{name} misround", r["misround"])
        record_property(f"{name} undecided", r["undecided"])
        record_property(f"{name} mean", r["mean"])
        assert r["wrong"] == 0, (kw, r)
        assert r["undecided"] <= P.UNDECIDED_MAX, (kw, r)


@pytest.mark.parametrize("src", ["ldr", "tonemapped"])
def test_post_ref_cas_meets_the_byte_rule(oracle, src, record_property):
    img = ldr(300, 400, 7) if src == "ldr" else oracle.tonemap(hdr_bits(300, 400, 5), exposure=0.9)
    for s in (0.0, 0.5, 1.0):
        x = P.cas64(img, s)
        dec, want = P.cas_decide(x)
        r = P.byte_check(P.channels(post_ref.cas(img, s)), dec, want, P.cas_bytes(x))
        record_property(f"s={s} misround", r["misround"])
        record_property(f"s={s} undecided", r["undecided"])
        record_property(f"s={s} mean", r["mean"])
        assert r["wrong"] == 0 and r["undecided"] <= P.UNDECIDED_MAX, (s, r)


def taa_frames(h, w, seed, brighter=False):
    rng = np.random.default_rng(seed)
    cur = (rng.random((h, w, 4)) ** 2 * 8).astype(np.float16)
    hist = ((rng.random((h, w, 4)) ** 2 * 8) if not brighter else cur.astype(np.float32) * 1.5 + 0.25).astype(np.float16)
    cur[..., 3] = 2.0
    return cur.view(np.uint16), hist.view(np.uint16)


@pytest.mark.parametrize("brighter", [False, True])
def test_oracle_temporal_aa_meets_r1_r3(oracle, brighter, record_property):
    cb, hb = taa_frames(67, 131, 9, brighter)
    for wt in (0.9, 0.35, 1.0):
        x, bound = P.temporal_aa64(cb, hb, wt, with_bound=True)
        m = P.measure(oracle.temporal_aa(cb, hb, wt, True), x, np.zeros(cb.shape[:2], bool))
        record_property(f"w={wt} misround", m["misround"])
        record_property(f"w={wt} mean_e", m["mean"])
        record_property(f"w={wt} max_e", float(np.nanmax(np.abs(m["e"]))))
        assert not P.r1_violations(m["e"], bound).any() and m["nan_mismatch"] == 0
        assert (np.abs(m["e"]) <= bound).all()  # the derived bound itself holds
        assert abs(m["mean"]) <= 0.02
        assert (bound > 1).mean() < 5e-3  # the cancellation allowance is rare


@pytest.mark.parametrize("h,w", [(1080 // 8, 1920 // 8), (9, 17), (1, 1), (1, 37), (37, 1), (15, 15), (16, 16), (17, 16)])
def test_post_ref_auto_exposure_within_tau(h, w, record_property):
    bits = hdr_bits(h, w, 11)
    img = post_ref.half4(bits)
    exact = P.auto_exposure64(bits)
    tau = P.ae_tau(bits)
    got = float(post_ref.auto_exposure(img))
    record_property("tau", tau)
    record_property("err", got - exact)
    assert abs(got - exact) <= tau, (got, exact, tau)
    assert tau < 5e-5  # the derived bound is tighter than the old 1e-4
    for prev in (exact - 1.5, exact + 1.5):
        kw = dict(prev=prev, use_history=True, delta_time=1 / 30, speed_up=3.0, speed_down=1.0)
        got = float(post_ref.auto_exposure(img, prev=F32(prev), use_history=True, delta_time=1 / 30))
        assert abs(got - P.auto_exposure64(bits, **kw)) <= P.ae_tau(bits, **kw)


# ---- planted errors: through the old tolerance, caught by the rules ---------------------------------------------------------
def _old_ok(got_rgb, ref_rgb):
    d = np.abs(np.asarray(got_rgb, np.int64) - np.asarray(ref_rgb, np.int64))
    return d.max() <= 1 and (d > 0).mean() < 2e-3


@pytest.mark.parametrize("plant", [dict(exposure_scale=1 + 1e-5), dict(desaturation=0.15001)])
def test_planted_tonemap_errors_fail_the_rule(oracle, plant, record_property):
    """A 1e-5 relative exposure bias, and desaturation 0.15 -> 0.15001. (0.15 -> 0.1503 moves 3e-2 of the cube fixture's bytes
    at exposure 1, so the old tolerance catches it already; 0.15001 is the size that passes it.)"""
    wrong = 0
    for bits in (cube_bits(384, 512, 4), hdr_bits(384, 512, 3)):
        for kw in (dict(exposure=1.0), dict(exposure=2.0), dict(exposure=0.9, gamma=1.0)):
            dec, want, _ = _tm_rule(bits, **kw)
            bad = P.tonemap_bytes(P.tonemap64(bits, **kw, **plant)[1])
            r = P.byte_check(bad, dec, want)
            record_property(f"{kw} wrong", r["wrong"])
            wrong += r["wrong"]
            assert _old_ok(bad, P.channels(oracle.tonemap(bits, **kw))), (kw, plant)
    assert wrong > 0, plant


def test_planted_cas_error_fails_the_rule(oracle, record_property):
    """FsrEps x 1.01."""
    for img in (ldr(300, 400, 7), oracle.tonemap(hdr_bits(300, 400, 5), exposure=0.9)):
        for s in (0.5, 1.0):
            x = P.cas64(img, s)
            dec, want = P.cas_decide(x)
            bad = P.cas_bytes(P.cas64(img, s, eps_scale=1.01))
            r = P.byte_check(bad, dec, want)
            record_property(f"s={s} wrong", r["wrong"])
            assert r["wrong"] > 0
            assert _old_ok(bad, P.channels(post_ref.cas(img, s)))


# an unstructured weight: with 0.9 the fp16 grid of c + 0.9 (max - c) is itself biased (-0.04 ulp correctly rounded)
TAA_W_BIAS = 0.7371


def test_planted_temporal_aa_error_fails_r3():
    """HistoryWeight x (1 + 2^-11): where the history sits above the box the blend moves up by w * (max - c) * 2^-11 - at most
    half an fp16 ulp, mostly far less - a bias R3 sees."""
    cb, hb = taa_frames(67, 131, 9, brighter=True)
    x, bound = P.temporal_aa64(cb, hb, TAA_W_BIAS, with_bound=True)
    bad = P.round16(P.temporal_aa64(cb, hb, TAA_W_BIAS, weight_scale=1 + 2.0 ** -11)).astype(np.float16).view(np.uint16)
    m = P.measure(bad, x, np.zeros(cb.shape[:2], bool))
    assert m["mean"] > 0.02, m["mean"]
    good = P.round16(x).astype(np.float16).view(np.uint16)
    assert abs(P.measure(good, x, np.zeros(cb.shape[:2], bool))["mean"]) <= 0.02
