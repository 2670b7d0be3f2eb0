"""Scalar numpy fp32 restatement of the post chain's AutoExposure and CAS, written from the HLSL (helper of
tests/test_post_abi.py and tests/test_gpu_post.py; no tests here).

AutoExposure: Shaders/AutoExposure.hlsl:24-93. SampleLevel(linear, clamp) of mip 0 is the 2x2 footprint around
t = uv * size - 0.5 with clamped indices, weights the fractions of t in fp32, blended as two lerps along x then one along y
(a + f * (b - a)); the sum runs in the kernel's fixed order (each wave a lane ^ 32, 16, ..., 1 butterfly, then the four wave
sums in index order).
CAS: Shaders/Cas.hlsl:67-99 with every tap an exact neighbour texel (TexelDelta = one texel at pixel centres), clamped at the
image edges; a texel is byte / 255; output saturated and rounded as round-half-up of x * 255 (the kernels' fmaf(x, 255, 0.5)).
"""
from __future__ import annotations

import numpy as np

F = np.float32
LUM = (F(0.2126), F(0.7152), F(0.0722))  # LuminanceWeights (AutoExposure.hlsl:33), LumCoeff (Cas.hlsl:54)


def half4(bits_u16: np.ndarray) -> np.ndarray:
    """(h, w, 4) uint16 RGBA16F bits -> float32 values."""
    return np.ascontiguousarray(bits_u16).view(np.float16).astype(F)


def _wave_sum(v: np.ndarray) -> F:
    """Lane 0's value after s += s[lane ^ m] for m = 32, 16, ..., 1 over 64 lanes."""
    s = v.astype(F).copy()
    idx = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        s = (s + s[idx ^ m]).astype(F)
    return F(s[0])


def ae_target_and_adapt(log_average_ev: F, prev=None, use_history=False, delta_time=0.0, speed_up=3.0, speed_down=1.0, key=0.3, ev_min=0.1,
                        ev_max=5.0) -> F:
    """AutoExposure.hlsl:76-92 from logAverageEv on."""
    key_ev = np.log2(np.maximum(F(key), F(1e-4)))
    min_ev, max_ev = np.log2(np.maximum(F(ev_min), F(1e-4))), np.log2(np.maximum(F(ev_max), F(1e-4)))
    target = np.minimum(np.maximum(F(key_ev - F(log_average_ev)), min_ev), max_ev)  # clamp(x, lo, hi) = min(max(x, lo), hi)
    adapted = F(target)
    if use_history:
        prev = F(prev)
        speed = F(speed_up) if target > prev else F(speed_down)
        alpha = F(F(1) - np.exp(F(-F(delta_time) * speed)))
        a = np.minimum(np.maximum(alpha, F(0)), F(1))  # saturate
        adapted = F(prev + F(a * F(target - prev)))  # lerp(prev, target, a)
    return F(adapted)


def auto_exposure_log_average(hdr: np.ndarray) -> F:
    """AutoExposure.hlsl:26-71: logAverageEv of a (h, w, 4) float32 frame (InputSize = (w, h))."""
    h, w = hdr.shape[:2]
    size_x, size_y = F(w), F(h)
    index = np.arange(256)
    gx, gy = (index & 15).astype(F), (index >> 4).astype(F)
    with np.errstate(invalid="ignore", over="ignore"):
        spx = ((gx + F(0.5)) * F(size_x / F(16))).astype(F)           # samplePos = groupCoord * (InputSize / 16)
        spy = ((gy + F(0.5)) * F(size_y / F(16))).astype(F)
        u = (spx / np.maximum(size_x, F(1))).astype(F)                # uv = samplePos / max(InputSize, 1)
        v = (spy / np.maximum(size_y, F(1))).astype(F)
        tx, ty = (u * size_x - F(0.5)).astype(F), (v * size_y - F(0.5)).astype(F)
        fx, fy = np.floor(tx), np.floor(ty)
        ax, ay = (tx - fx).astype(F), (ty - fy).astype(F)
        ix, iy = fx.astype(np.int64), fy.astype(np.int64)
        x0, x1 = np.clip(ix, 0, w - 1), np.clip(ix + 1, 0, w - 1)
        y0, y1 = np.clip(iy, 0, h - 1), np.clip(iy + 1, 0, h - 1)
        t00, t10, t01, t11 = hdr[y0, x0, :3], hdr[y0, x1, :3], hdr[y1, x0, :3], hdr[y1, x1, :3]
        axc, ayc = ax[:, None], ay[:, None]
        top = (t00 + axc * (t10 - t00)).astype(F)
        bottom = (t01 + axc * (t11 - t01)).astype(F)
        c = (top + ayc * (bottom - top)).astype(F)
        cm = np.fmax(c, F(0))  # max(color, 0) with a NaN channel -> 0
        lum = ((cm[:, 0] * LUM[0] + cm[:, 1] * LUM[1]).astype(F) + cm[:, 2] * LUM[2]).astype(F)
        logv = np.log2(np.maximum(lum, F(1e-4))).astype(F)
    sums = [_wave_sum(logv[64 * k:64 * (k + 1)]) for k in range(4)]
    total = F(F(F(sums[0] + sums[1]) + sums[2]) + sums[3])
    return F(total / F(256))


def auto_exposure(hdr: np.ndarray, prev=None, use_history=False, delta_time=0.0, speed_up=3.0, speed_down=1.0, key=0.3, ev_min=0.1,
                  ev_max=5.0) -> F:
    """The float AutoExposure.hlsl writes to LogAverageLuminance[0, 0] for a (h, w, 4) float32 frame."""
    return ae_target_and_adapt(auto_exposure_log_average(hdr), prev, use_history, delta_time, speed_up, speed_down, key, ev_min, ev_max)


def unorm8(x: np.ndarray) -> np.ndarray:
    """saturate, then fmaf(x, 255, 0.5) truncated (x * 255 + 0.5 is exact in float64: one rounding to float32, like the fma)."""
    x = np.minimum(np.maximum(x.astype(F), F(0)), F(1))
    return (x.astype(np.float64) * 255.0 + 0.5).astype(F).astype(np.uint32)


def cas(ldr: np.ndarray, sharpness: float, row0: int = 0, rows: int | None = None) -> np.ndarray:
    """Cas.hlsl:67-99 over rows [row0, row0 + rows) of a (h, w) uint32 R8G8B8A8 image -> (rows, w) uint32 (A = 255)."""
    h, w = ldr.shape
    rows = h - row0 if rows is None else rows
    rgb = ((ldr[..., None] >> np.array([0, 8, 16], np.uint32)) & 255).astype(F) / F(255)
    y = np.arange(row0, row0 + rows)
    x = np.arange(w)
    C = rgb[y]
    N = rgb[np.clip(y - 1, 0, h - 1)]
    S = rgb[np.clip(y + 1, 0, h - 1)]
    W = C[:, np.clip(x - 1, 0, w - 1)]
    E = C[:, np.clip(x + 1, 0, w - 1)]

    def dot(c):
        return ((c[..., 0] * LUM[0] + c[..., 1] * LUM[1]).astype(F) + c[..., 2] * LUM[2]).astype(F)

    CL, NL, WL, EL, SL = dot(C), dot(N), dot(W), dot(E), dot(S)
    rcas_inv_peak, eps = F(1) / F(8 - 3), F(0.0001)
    mn = np.minimum(np.minimum(np.minimum(N, W), np.minimum(E, S)), C)
    mx = np.maximum(np.maximum(np.maximum(N, W), np.maximum(E, S)), C)
    inv_max = (F(1) / (mx + eps)).astype(F)
    amp = np.clip((np.minimum(mn, F(2) - mx) * inv_max).astype(F), F(0), F(1))
    amp = (F(1) / np.sqrt(amp + eps)).astype(F)                      # rsqrt
    wgt = (-rcas_inv_peak / dot(amp)).astype(F)
    sum_l = (((NL + WL) + EL) + SL).astype(F)
    inv_den = (F(1) / (F(4) * wgt + F(1))).astype(F)
    sharp_l = np.clip(((sum_l * wgt + CL) * inv_den).astype(F), F(0), F(1))
    sharp_color = ((C - CL[..., None]) + sharp_l[..., None]).astype(F)
    out = (C + F(sharpness) * (sharp_color - C)).astype(F)           # lerp(C, sharpColor, Sharpness)
    q = unorm8(out)
    return q[..., 0] | (q[..., 1] << 8) | (q[..., 2] << 16) | np.uint32(0xFF000000)


def bytes_of(img_u32: np.ndarray) -> np.ndarray:
    """(..., 4) uint8 view of packed R8G8B8A8 words."""
    return np.ascontiguousarray(img_u32).view(np.uint8).reshape(img_u32.shape + (4,))
