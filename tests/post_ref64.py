"""Vectorised numpy float64 restatement of the post chain - Tonemap, CAS, TemporalAA and AutoExposure - written from the HLSL,
and the rules that decide whether an 8-bit, fp16 or EV result of a kernel is right (helper of tests/test_post_ref64.py and
tests/test_gpu_post_accuracy.py; no tests here).

  * Tonemap: Shaders/Tonemap.hlsl:34-79 (exposure [x 2^EV], PBRNeutralToneMapping, saturate, gamma).
  * CAS: Shaders/Cas.hlsl:67-99 from the input bytes, every tap the exact neighbour texel clamped at the image edges (as
    tests/post_ref.py:cas).
  * TemporalAA: Shaders/TemporalAA.hlsl:12-50 (3x3 box of the current frame, history clamped into it, lerp).
  * AutoExposure: Shaders/AutoExposure.hlsl:24-93 (16 x 16 bilinear taps at t = (g + 0.5) * size / 16 - 0.5, the mean of
    log2(max(luminance, 1e-4)), key / clamp, adaptation).
Conventions, as in tests/lighting_ref64.py: a shader literal is the fp32 value the compiled shader holds, widened exactly
(`_c`); min / max ignore a NaN operand (HLSL's min / max, np.fmin / np.fmax); saturate(NaN) = 0. Every operation runs in
float64, so what comes back is the exact value the kernel's one quantisation (8-bit or fp16) should round.

The decision rules and their budgets
------------------------------------
u = 2^-24 is the unit roundoff of fp32; a rounded fp32 operation (-ffp-contract=off: no fused pairs the source does not spell)
adds a relative error of at most u, and v_rcp_f32 / v_rsq_f32 / v_log_f32 / v_exp_f32 (1 ulp) at most 2u.

BYTES (Tonemap, CAS). A byte is DECIDED when round_half_up(v * 255) is the same integer at both ends of the interval
[x - eps, x + eps], eps = a + r * |x|, pushed through what follows x (saturate, and for Tonemap the exact gamma curve and a
relative budget for it); only decided bytes are held to the exact answer, and the undecided fraction is reported (and capped
by the tests, so the budgets cannot grow into meaninglessness).

  Tonemap, x = the linear value before saturate (TM_A, TM_R):
    exposure: v_exp_f32 (2u) and the product with Exposure (u); colour = hdr * exposure (u)          -> 4u relative
    offset x - 6.25 x^2 (two roundings, x in [0, 0.08)) and colour - offset: on the min channel the subtraction cancels
      to 6.25 x^2, leaving an absolute error of a few u * 0.08                                        -> 4u relative + 2^-26 abs
    compression (peak >= 0.76): peak + d - start (2u), v_rcp (2u), d * d and the product (2u) give newPeak within 2^-23
      absolute; s = newPeak * v_rcp(peak) (4u + peak's 4u) and colour * s (u): relative 14u on values <= 1; the
      desaturation weight 1 - v_rcp(0.15 * (peak - newPeak) + 1): peak - newPeak cancels, its 2^-21 * peak absolute error
      is divided by the square of the denominator (>= 1 + 0.15 peak - 0.15), plus 2u of v_rcp and u of the subtraction:
      <= 2^-21 absolute; the lerp fmaf(g, newPeak - c, c) adds 2u of its own                        -> 2^-20 abs, 16u rel
    so TM_A = 2^-20 where the compression runs (TM_A_LIN = 2^-26 where it does not) and TM_R = 2^-20 (16u).
    gamma, the kernel's exp2(e * log2 y) against the exact y^e (TM_RG): log2 within 2u relative of log2 y, the product
    u, so the exponent e * log2 y = log2 v is off by 3u * |log2 v|; v_exp_f32 adds 2u, and the 8-bit rounding's fmaf
    x * 255 + 0.5 one rounding of a value <= 256 (2^-16 of a byte, < u relative above byte 1). A byte above 0 needs
    v >= 2^-9, |log2 v| <= 9: 27 ln 2 u + 2u + u < 22u; TM_RG = 2^-18 (64u) leaves the factor 3 for the oracle's powf.
  CAS, x = the value before the output saturate (CAS_A, CAS_R): the texels byte * (1/255) (2u), luminance (3 products, 2
    sums: 5u of a value <= 1); amp: 2 - max (u), the product with v_rcp(max + eps) (3u), saturate, + eps (u), v_rsq (2u):
    amp (<= 100) within 8u relative; the weight -0.2 * v_rcp(sum of 3 products amp * lum) within 10u relative of w in
    [-0.2, 0); sumL (3 sums of values <= 1: 3u * 4), sumL * w + CL (cancels: absolute 2^-22), v_rcp(4w + 1) (den >= 0.2,
    4u relative, + 5 * 10u * 0.8 / 0.2 from w): sharpL within 2^-19 absolute; the output C + s * ((C - CL) + sharpL - C)
    (4 roundings of values <= 2, 2^-21)                                                                 -> CAS_A = 2^-18 (x2)
    CAS_R = 0: every error above is absolute, on values bounded by 2.

FP16 (TemporalAA). The kernel clamps (exact) and blends in fp32 and rounds once to fp16: R1 (|e| <= 1 ulp of the exact value,
or the yardstick taa_bound + 1 where the fp32 blend's cancellation makes that larger: see TAA_U) and R3 (mean signed error
within +-0.02 ulp) of tests/lighting_ref64.py, which this module imports rather than restates.

EV (AutoExposure). |got - exact| <= tau_ae, with tau_ae computed for the frame from the instruction bounds (ae_tau below):
the tap coordinate t = (2g + 1) * size / 32 - 0.5 is exact in fp32 at every size below 2^24 / 31 (above, its four
roundings move it by at most 4u * size, and a bilinear tap is Lipschitz in t with the largest texel difference around it); three lerps (9 roundings) and the luminance (5) add 14u of the largest texel;
log2 turns an error dL into dL / (ln 2 * max(L - dL, 1e-4)), plus 2u * |log2 L| of log2f itself; the fixed-order sum of 256
values <= 13.3 in magnitude adds at most 9 roundings of partial sums (6 in the wave butterfly, 3 across the waves); the key,
min and max EVs 2u of their log2 each, the subtraction u; the history step (alpha = 1 - exp(-dt * speed): 4u absolute, the
lerp 3 roundings) adds 4u * |target - prev| + 3u * max(|prev|, |target|).
"""
from __future__ import annotations

import warnings

import numpy as np

from tests.lighting_ref64 import _c, measure, r1_violations, round16, signed_error, ulp16  # noqa: F401  (re-exported)

F64 = np.float64
F32 = np.float32
U = 2.0 ** -24

TM_A = 2.0 ** -20      # absolute, where the compression branch runs
TM_A_LIN = 2.0 ** -26  # absolute, where it does not
TM_R = 2.0 ** -20      # relative, the linear value
TM_RG = 2.0 ** -18     # relative, the gamma stage (the kernel's exp2(e * log2 y), the oracle's powf)
CAS_A = 2.0 ** -18     # absolute, the value before the output saturate
CAS_R = 0.0
UNDECIDED_MAX = 5e-3   # the tests' cap on the undecided fraction

LUM = (_c(0.2126), _c(0.7152), _c(0.0722))  # LuminanceWeights (AutoExposure.hlsl:33), LumCoeff (Cas.hlsl:54)


def _sat(x):
    """saturate(): NaN -> 0."""
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(x), 0.0, np.clip(x, 0.0, 1.0))


def _dot3(c):
    return c[..., 0] * LUM[0] + c[..., 1] * LUM[1] + c[..., 2] * LUM[2]


def round_half_up(v):
    """The 8-bit UNORM of v * 255 with v already saturated: floor(v * 255 + 0.5) (the kernels' fmaf(v, 255, 0.5), truncated)."""
    return np.floor(np.asarray(v, F64) * 255.0 + 0.5).astype(np.int64)


def hdr64(bits_u16: np.ndarray) -> np.ndarray:
    """(..., 4) uint16 RGBA16F bits -> float64 values (signalling NaN patterns become NaN)."""
    return np.ascontiguousarray(bits_u16, np.uint16).view(np.float16).astype(F64)


def channels(img_u32: np.ndarray) -> np.ndarray:
    """(...) uint32 R8G8B8A8 -> (..., 3) int64 R, G, B."""
    return ((np.asarray(img_u32, np.uint32)[..., None] >> np.array([0, 8, 16], np.uint32)) & 255).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------------
# Tonemap
# ---------------------------------------------------------------------------------------------------------------------
def inv_gamma(gamma) -> F64:
    """The fp32 1 / max(Gamma, 1e-3) both the pass and the kernels compute, widened."""
    return F64(F32(1.0) / max(F32(gamma), F32(1e-3)))


def tonemap64(hdr_bits, exposure=1.0, gamma=2.2, enable_tonemap=True, exposure_ev=None, exposure_scale=1.0, desaturation=0.15):
    """Tonemap.hlsl:57-79 of (..., 4) RGBA16F bits. Returns (lin, v255, compressed): the exact linear value before saturate
    ((..., 3)), the exact pow(saturate(lin), invGamma) * 255 ((..., 3)) and where the compression branch ran ((...)).
    exposure_scale / desaturation exist to plant errors; the shader's are 1 and 0.15."""
    c = hdr64(hdr_bits)[..., :3]
    fe = _c(exposure) * (2.0 ** F64(F32(exposure_ev)) if exposure_ev is not None else 1.0) * exposure_scale
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        c = c * fe
        comp = np.zeros(c.shape[:-1], bool)
        if enable_tonemap:  # PBRNeutralToneMapping, Tonemap.hlsl:34-55
            start = F64(F32(0.8) - F32(0.04))
            desat = _c(desaturation)
            x = np.fmin(c[..., 0], np.fmin(c[..., 1], c[..., 2]))
            offset = np.where(x < _c(0.08), x - _c(6.25) * x * x, _c(0.04))
            c = c - offset[..., None]
            peak = np.fmax(c[..., 0], np.fmax(c[..., 1], c[..., 2]))
            comp = ~(peak < start)
            d = 1.0 - start
            new_peak = 1.0 - d * d / (peak + d - start)
            s = new_peak / np.fmax(peak, _c(1e-4))
            g = 1.0 - 1.0 / (desat * (peak - new_peak) + 1.0)
            cc = c * s[..., None]
            cc = cc + g[..., None] * (new_peak[..., None] - cc)  # lerp(color, newPeak, g)
            c = np.where(comp[..., None], cc, c)
        v = np.power(_sat(c), inv_gamma(gamma)) * 255.0
    return c, v, comp


def tonemap_bytes(v255) -> np.ndarray:
    """The exact 8-bit result of tonemap64's v255."""
    return np.minimum(round_half_up(np.asarray(v255) / 255.0), 255)


def tonemap_decide(lin, comp, gamma) -> tuple[np.ndarray, np.ndarray]:
    """(decided, byte) per channel of tonemap64's output under the budgets TM_A / TM_A_LIN, TM_R, TM_RG."""
    lin = np.asarray(lin, F64)
    a = np.where(np.asarray(comp)[..., None], TM_A, TM_A_LIN)
    with np.errstate(invalid="ignore", over="ignore"):
        eps = a + TM_R * np.abs(lin)
        e = inv_gamma(gamma)
        lo = np.power(_sat(lin - eps), e) * (1.0 - TM_RG)
        hi = np.minimum(np.power(_sat(lin + eps), e) * (1.0 + TM_RG), 1.0)
    blo, bhi = round_half_up(lo), round_half_up(hi)
    nan = np.isnan(lin)  # saturate(NaN) = 0 whatever the error: decided, byte 0
    return (blo == bhi) | nan, np.where(nan, 0, blo)


# ---------------------------------------------------------------------------------------------------------------------
# CAS
# ---------------------------------------------------------------------------------------------------------------------
def cas64(ldr: np.ndarray, sharpness: float, row0: int = 0, rows: int | None = None, eps_scale=1.0):
    """Cas.hlsl:67-99 over rows [row0, row0 + rows) of a (h, w) uint32 R8G8B8A8 image. Returns the exact RGB before the output
    saturate ((rows, w, 3) float64). eps_scale exists to plant an error (the shader's is 1)."""
    h, w = ldr.shape
    rows = h - row0 if rows is None else rows
    rgb = channels(ldr).astype(F64) / 255.0
    y = np.arange(row0, row0 + rows)
    x = np.arange(w)
    C = rgb[y]
    N = rgb[np.clip(y - 1, 0, h - 1)]
    S = rgb[np.clip(y + 1, 0, h - 1)]
    W = C[:, np.clip(x - 1, 0, w - 1)]
    E = C[:, np.clip(x + 1, 0, w - 1)]
    eps = _c(0.0001) * eps_scale
    rcas_inv_peak = _c(1.0 / (8.0 - 3.0))
    mn = np.minimum(np.minimum(np.minimum(N, W), np.minimum(E, S)), C)
    mx = np.maximum(np.maximum(np.maximum(N, W), np.maximum(E, S)), C)
    amp = _sat(np.minimum(mn, 2.0 - mx) * (1.0 / (mx + eps)))
    amp = 1.0 / np.sqrt(amp + eps)
    wgt = -rcas_inv_peak / _dot3(amp)
    sum_l = _dot3(N) + _dot3(W) + _dot3(E) + _dot3(S)
    sharp_l = _sat((sum_l * wgt + _dot3(C)) / (4.0 * wgt + 1.0))
    sharp_color = (C - _dot3(C)[..., None]) + sharp_l[..., None]
    return C + _c(sharpness) * (sharp_color - C)


def cas_bytes(x) -> np.ndarray:
    return round_half_up(_sat(np.asarray(x, F64)))


def cas_decide(x) -> tuple[np.ndarray, np.ndarray]:
    """(decided, byte) per channel of cas64's output under CAS_A / CAS_R."""
    x = np.asarray(x, F64)
    eps = CAS_A + CAS_R * np.abs(x)
    lo, hi = cas_bytes(x - eps), cas_bytes(x + eps)
    return lo == hi, lo


# ---------------------------------------------------------------------------------------------------------------------
# the byte rule, summarised
# ---------------------------------------------------------------------------------------------------------------------
def byte_check(got_rgb, decided, want, exact_bytes=None, ref_rgb=None) -> dict:
    """got_rgb / want: (..., 3) integer bytes; decided: (..., 3) bool. Returns the counts of the rule: wrong (decided bytes that
    differ from `want`), undecided (fraction), and, given the exact bytes, misround (fraction of all bytes != exact) and mean
    (signed mean of got - exact over all bytes); given a yardstick ref_rgb, the old rule's max LSB and off fraction."""
    got_rgb = np.asarray(got_rgb, np.int64)
    r = dict(n=int(decided.size), wrong=int((decided & (got_rgb != want)).sum()), undecided=float(1.0 - decided.mean()))
    if exact_bytes is not None:
        r["misround"] = float((got_rgb != exact_bytes).mean())
        r["mean"] = float((got_rgb - exact_bytes).mean())
    if ref_rgb is not None:
        dd = np.abs(got_rgb - np.asarray(ref_rgb, np.int64))
        r["old_max"], r["old_off"] = int(dd.max()), float((dd > 0).mean())
    return r


# ---------------------------------------------------------------------------------------------------------------------
# TemporalAA
# ---------------------------------------------------------------------------------------------------------------------
def temporal_aa64(current_bits, history_bits, history_weight, row0=0, rows=None, pixels=None, weight_scale=1.0, with_bound=False):
    """TemporalAA.hlsl:12-50 with history: the exact c + w * (clamp(h, min9, max9) - c) of band rows [row0, row0 + rows)
    ((rows, W, 4) float64; alpha is the current texel's). current_bits: (H, W, 4) full frame; history_bits: (rows, W, 4) band.
    pixels: optional (ys, xs) band coordinates -> (n, 4). weight_scale exists to plant an error.
    with_bound: also return taa_bound's per-value bound (same shape)."""
    cur = hdr64(current_bits)
    H, W = cur.shape[:2]
    rows = H - row0 if rows is None else rows
    if pixels is None:
        ys, xs = np.mgrid[0:rows, 0:W]
        ys, xs = ys.ravel(), xs.ravel()
    else:
        ys, xs = (np.asarray(p, np.int64) for p in pixels)
    hist = hdr64(history_bits)[ys, xs]
    fy = ys + row0
    c = cur[fy, xs]
    mn, mx = c[:, :3].copy(), c[:, :3].copy()
    for oy in (-1, 0, 1):
        for ox in (-1, 0, 1):
            s = cur[np.clip(fy + oy, 0, H - 1), np.clip(xs + ox, 0, W - 1), :3]
            mn, mx = np.fmin(mn, s), np.fmax(mx, s)
    wt = F64(F32(history_weight))
    w = 0.0 if np.isnan(wt) else min(max(wt, 0.0), 1.0)
    w *= weight_scale
    with np.errstate(invalid="ignore"):
        hc = np.fmin(np.fmax(hist[:, :3], mn), mx)
        out = np.empty((len(ys), 4), F64)
        out[:, :3] = c[:, :3] + w * (hc - c[:, :3])
    out[:, 3] = c[:, 3]
    shape = (lambda a: a) if pixels is not None else (lambda a: a.reshape(rows, W, 4))
    if not with_bound:
        return shape(out)
    bound = np.full(out.shape, 0.5)
    with np.errstate(invalid="ignore"):
        big = np.fmax(np.abs(c[:, :3]), np.abs(hc))
        bound[:, :3] = 0.5 + TAA_U * big / ulp16(out[:, :3])
    return shape(out), shape(bound)


# The kernel's fp32 blend c + w * (h - c) rounds three times (the difference, the product, the sum), each by at most u of a
# value no larger than max(|c|, |h|): 3u * max(|c|, |h|) before the one fp16 rounding (0.5 ulp). Where the result is far
# smaller than c (the history pulls a bright texel dark) that term exceeds half an fp16 ulp of the result: taa_bound is the
# per-value bound 0.5 + TAA_U * max(|c|, |h|) / ulp16(x) in ulps, and R1 (r1_violations with it as the yardstick) allows it.
TAA_U = 3 * U


# ---------------------------------------------------------------------------------------------------------------------
# AutoExposure
# ---------------------------------------------------------------------------------------------------------------------
def _ae_taps(h, w):
    """The exact tap coordinates t = (g + 0.5) * size / 16 - 0.5 of the 256 lanes (index = gy * 16 + gx)."""
    index = np.arange(256)
    gx, gy = (index & 15).astype(F64), (index >> 4).astype(F64)
    return (gx + 0.5) * w / 16.0 - 0.5, (gy + 0.5) * h / 16.0 - 0.5


def _ae_tap_values(hdr, tx, ty):
    h, w = hdr.shape[:2]
    fx, fy = np.floor(tx), np.floor(ty)
    ax, ay = (tx - fx)[:, None], (ty - fy)[:, None]
    ix, iy = fx.astype(np.int64), fy.astype(np.int64)
    x0, x1 = np.clip(ix, 0, w - 1), np.clip(ix + 1, 0, w - 1)
    y0, y1 = np.clip(iy, 0, h - 1), np.clip(iy + 1, 0, h - 1)
    t00, t10, t01, t11 = hdr[y0, x0, :3], hdr[y0, x1, :3], hdr[y1, x0, :3], hdr[y1, x1, :3]
    with np.errstate(invalid="ignore", over="ignore"):
        top = t00 + ax * (t10 - t00)
        bottom = t01 + ax * (t11 - t01)
        return top + ay * (bottom - top), (x0, y0)


def _ae_lum(c):
    cm = np.fmax(c, 0.0)  # max(color, 0): a NaN channel counts as 0
    return _dot3(cm)


def ae_log_average64(hdr_bits) -> F64:
    """AutoExposure.hlsl:26-71: the exact logAverageEv of a (h, w, 4) RGBA16F frame (InputSize = (w, h))."""
    hdr = hdr64(hdr_bits)
    h, w = hdr.shape[:2]
    tx, ty = _ae_taps(h, w)
    c, _ = _ae_tap_values(hdr, tx, ty)
    with np.errstate(divide="ignore", invalid="ignore"):
        return F64(np.log2(np.fmax(_ae_lum(c), _c(1e-4))).sum() / 256.0)


def _ae_bounds(key, ev_min, ev_max):
    lg = lambda v: np.log2(max(_c(v), _c(1e-4)))
    return lg(key), lg(ev_min), lg(ev_max)


def ae_adapt64(log_average_ev, prev=None, use_history=False, delta_time=0.0, speed_up=3.0, speed_down=1.0, key=0.3, ev_min=0.1,
               ev_max=5.0) -> F64:
    """AutoExposure.hlsl:76-92 from the exact logAverageEv on: the exact adapted EV."""
    key_ev, min_ev, max_ev = _ae_bounds(key, ev_min, ev_max)
    with np.errstate(invalid="ignore"):
        target = F64(np.fmin(np.fmax(key_ev - F64(log_average_ev), min_ev), max_ev))
    if not use_history:
        return target
    prev = F64(F32(prev))
    speed = _c(speed_up) if target > prev else _c(speed_down)
    alpha = 1.0 - np.exp(-_c(delta_time) * speed)
    return F64(prev + float(_sat(alpha)) * (target - prev))


def auto_exposure64(hdr_bits, **kw) -> F64:
    return ae_adapt64(ae_log_average64(hdr_bits), **kw)


def ae_tau(hdr_bits, prev=None, use_history=False, delta_time=0.0, speed_up=3.0, speed_down=1.0, key=0.3, ev_min=0.1, ev_max=5.0) -> float:
    """tau_ae for this frame and these constants: the bound on |kernel - exact| derived in the module docstring."""
    hdr = hdr64(hdr_bits)
    h, w = hdr.shape[:2]
    tx, ty = _ae_taps(h, w)
    c, (x0, y0) = _ae_tap_values(hdr, tx, ty)
    # the neighbourhood a tap coordinate off by dt can reach: columns x0 - 1 .. x0 + 2, rows y0 - 1 .. y0 + 2
    dx = np.stack([np.clip(x0 + k, 0, w - 1) for k in (-1, 0, 1, 2)], 1)
    dy = np.stack([np.clip(y0 + k, 0, h - 1) for k in (-1, 0, 1, 2)], 1)
    nb = hdr[dy[:, :, None], dx[:, None, :], :3].reshape(256, 16, 3)
    with np.errstate(invalid="ignore", over="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # an all-NaN neighbourhood: its tap is non-finite, handled below
        big = np.nanmax(np.abs(nb), axis=1)                       # largest texel per channel
        spread = np.nanmax(nb, axis=1) - np.nanmin(nb, axis=1)   # Lipschitz constant of the tap in t (per texel of t)
        # the tap coordinate: samplePos = (g + 0.5) * (size / 16) = (2g + 1) * size / 32, uv = samplePos / size = (2g + 1) / 32 and
        # t = uv * size - 0.5 are all exact in fp32 while 31 * size < 2^24; above, four roundings of values <= size
        dt = 0.0 if 31 * max(h, w) < 2 ** 24 else 4 * U * max(h, w)
        dc = dt * 2 * spread + 14 * U * big                      # both coordinates, and the lerps' roundings
        L = _ae_lum(c)
        dL = _dot3(dc) + 5 * U * np.abs(L)
        lo = np.fmax(L - dL, _c(1e-4))
        dlog = dL / (np.log(2.0) * lo) + 2 * U * np.abs(np.log2(np.fmax(L, _c(1e-4))))
    finite = np.isfinite(dlog) & np.isfinite(L)
    if not finite.all():
        # a non-finite tap: the sum is +-Inf or NaN and the clamp decides; only the constants' errors remain
        tap = 0.0
    else:
        tap = float(dlog.sum() / 256.0)
    summ = 9 * U * 256 * 13.3 / 256.0                             # 9 roundings of partial sums <= 256 * 13.3
    key_ev, min_ev, max_ev = _ae_bounds(key, ev_min, ev_max)
    const = 2 * U * (abs(key_ev) + abs(min_ev) + abs(max_ev)) + U * (abs(key_ev) + 13.3)
    tau = tap + summ + const
    if use_history:
        target = ae_adapt64(ae_log_average64(hdr_bits), key=key, ev_min=ev_min, ev_max=ev_max)
        p = float(F32(prev))
        tau += 4 * U * abs(target - p) + 3 * U * max(abs(p), abs(target))
    return tau
