"""Edge and special-value inputs for Lighting and Sky, and fp32 emulations of the kernels' decision forms (helper of
tests/test_lighting_edges.py and tests/test_gpu_lighting_edges.py; no tests here).

The semantics are the shaders' (DeferredLighting.hlsl:55-70, SkyAtmosphere.hlsl), as oracle/ur_oracle.cpp and
tests/lighting_ref64.py state them:
  * a PCF tap passes when cmp <= t (LESS_EQUAL): a NaN on either side fails;
  * a tap outside the map reads the opaque-white border, depth 1.0, and is compared like any other;
  * the sky is drawn where sphereDepth >= the stored depth (GREATER_EQUAL): a NaN depth is not sky, a depth <= 0 is.

The emulations restate, in exact arithmetic rounded once to fp32 where the instruction rounds, what csrc/lighting.hip and csrc/lighting_tiled.hip compute for
those decisions, and a few plain mutants next to them. The hardware clamp is assumed to send NaN to 0 (DX10 clamp).
"""
from __future__ import annotations

import struct
from fractions import Fraction

import numpy as np

F32 = np.float32


# ---------------------------------------------------------------------------------------------------------------------
# exact fp32 arithmetic on scalars
# ---------------------------------------------------------------------------------------------------------------------
def f32(bits: int) -> float:
    """The fp32 value of a bit pattern, widened to a Python float (NaN payloads are not kept)."""
    return float(np.uint32(bits).view(F32))


QNAN_BITS, SNAN_BITS = 0x7FC00000, 0x7F800001
TINY = f32(1)             # 2^-149, the smallest subnormal
NORM_MIN = f32(0x00800000)  # 2^-126


def round32(x: Fraction) -> float:
    """x rounded to nearest-even fp32 (overflow to +-Inf), as a Python float."""
    if x == 0:
        return 0.0
    mag = abs(x)
    if mag >= Fraction(2) ** 128 - Fraction(2) ** 103:  # half an ulp above FLT_MAX rounds to Inf
        return float("inf") if x > 0 else float("-inf")
    c = F32(float(x))  # float64 rounding then fp32: may round twice; fixed below with the exact neighbours
    best = None
    for cand in (np.nextafter(c, F32(-np.inf)), c, np.nextafter(c, F32(np.inf))):
        if not np.isfinite(cand):
            continue
        d = abs(Fraction(float(cand)) - x)
        key = (d, int(np.asarray(cand).view(np.uint32)) & 1)  # ties: the even mantissa
        if best is None or key < best[0]:
            best = (key, float(cand))
    return best[1]


def fma32(a: float, b: float, c: float) -> float:
    """fp32 fma with one rounding (inputs are fp32 values); IEEE rules for NaN and Inf."""
    if any(np.isnan(v) for v in (a, b, c)):
        return float("nan")
    if any(np.isinf(v) for v in (a, b, c)):
        return float(np.float64(a) * np.float64(b) + np.float64(c))
    return round32(Fraction(a) * Fraction(b) + Fraction(c))


def clamp01(x: float) -> float:
    """The VALU clamp bit: [0, 1], NaN -> 0 (DX10 clamp)."""
    return 0.0 if np.isnan(x) else min(max(x, 0.0), 1.0)


def pred32(x: float) -> float:
    return float(np.nextafter(F32(x), F32(-np.inf)))


# ---------------------------------------------------------------------------------------------------------------------
# one PCF tap: pass = 1.0, fail = 0.0
# ---------------------------------------------------------------------------------------------------------------------
def tap_hlsl(cmp: float, t: float) -> float:
    return 1.0 if cmp <= t else 0.0


def tap_step_le_v1(cmp: float, t: float) -> float:
    """The per-tile kernel's former step_le: saturate((t - cmp) * 2^126 + 1)."""
    return clamp01(fma32(round32(Fraction(t) - Fraction(cmp)) if np.isfinite(t) and np.isfinite(cmp) else t - cmp, 2.0 ** 126, 1.0))


def tap_gt_step_v1(cmp: float, t: float) -> float:
    """The streaming kernel's former gt_step: fail = clamp(cmp * 2^126 - t * 2^126), the tap is 1 - fail."""
    cb = round32(Fraction(cmp) * 2 ** 126) if np.isfinite(cmp) else cmp * 2.0 ** 126
    return 1.0 - clamp01(fma32(t, -(2.0 ** 126), cb))


def cmp_step_exact(cmp: float) -> bool:
    return 2.0 ** -100 <= abs(cmp) < 2.0  # False for NaN


def neg_pred_big(cmp: float) -> float:
    """-pred(cmp) * 2^126 as the streaming kernel forms it: fma(|cmp|, 2^-24 + 2^-47, -cmp) * 2^126."""
    return round32(Fraction(fma32(abs(cmp), 2.0 ** -24 + 2.0 ** -47, -cmp)) * 2 ** 126)


def tap_le_step(cmp: float, t: float) -> float:
    """The streaming kernel's le_step where cmp_step_exact holds, the compare elsewhere (its slow path)."""
    if not cmp_step_exact(cmp):
        return tap_hlsl(cmp, t)
    return clamp01(fma32(-t, -(2.0 ** 126), neg_pred_big(cmp)))


def tap_lt(cmp, t):  # mutant: LESS for LESS_EQUAL
    return 1.0 if cmp < t else 0.0


def tap_nan_passes(cmp, t):  # mutant: an unordered compare passes
    return 1.0 if (cmp <= t or np.isnan(cmp) or np.isnan(t)) else 0.0


TAP_FORMS = {"step_le (per-tile, before)": tap_step_le_v1, "gt_step (streaming, before)": tap_gt_step_v1,
             "le_step (streaming)": tap_le_step, "step_le (per-tile)": tap_hlsl, "mutant <": tap_lt, "mutant NaN passes": tap_nan_passes}
FIXED_TAP_FORMS = ("le_step (streaming)", "step_le (per-tile)")


# the border tap (outside the map): the texel is the border depth 1.0
def border_hlsl(cmp):
    return tap_hlsl(cmp, 1.0)


def border_always_passes(cmp):  # the streaming kernel's former shadow_pcf_border_inline
    return 1.0


BORDER_FORMS = {"border always passes (streaming, before)": border_always_passes, "border compared": border_hlsl}


# ---------------------------------------------------------------------------------------------------------------------
# the sky test: sphere depth against the stored depth
# ---------------------------------------------------------------------------------------------------------------------
def sky_hlsl(sphere: float, depth: float) -> bool:
    return sphere >= depth


def sky_squared_v1(sphere: float, depth: float) -> bool:
    """The fused streaming kernel's former test: sphere^2 >= depth^2 (fp32 squares)."""
    s2 = round32(Fraction(sphere) ** 2) if np.isfinite(sphere) else sphere * sphere
    d2 = round32(Fraction(depth) ** 2) if np.isfinite(depth) else depth * depth
    return s2 >= d2


def sky_squared(sphere: float, depth: float) -> bool:
    """The fused streaming kernel's test: depth <= 0, or the squares compared."""
    return depth <= 0.0 or sky_squared_v1(sphere, depth)


def sky_gt(sphere, depth):  # mutant: GREATER for GREATER_EQUAL
    return sphere > depth


SKY_FORMS = {"squared (streaming, before)": sky_squared_v1, "sign-aware squared (streaming)": sky_squared, "mutant >": sky_gt}


def window_hlsl(u: float) -> bool:
    return 0.0 <= u <= 1.0


def window_strict(u: float) -> bool:  # mutant: the window compared with <
    return 0.0 < u < 1.0


# ---------------------------------------------------------------------------------------------------------------------
# point sets
# ---------------------------------------------------------------------------------------------------------------------
SPECIAL_TEXEL_BITS = [QNAN_BITS, SNAN_BITS, 0x7F800000, 0xFF800000, 0x00000000, 0x80000000, 0x00000001, 0x80000001,
                      0x00800000, 0x80800000]
SPECIAL_TEXELS = [f32(b) for b in SPECIAL_TEXEL_BITS] + [float(F32(v)) for v in (4.0, 8.0, 10.0, 1e30, -4.0, -10.0, 0.5, 1.0)]
SHADOW_BIASES = (-1.5, -4.0, -8.0, 5.0)
SPECIAL_DEPTH_BITS = [0xBF800000, 0x80000000, 0x00000000, 0x00000001, 0x40000000, 0x7F800000, QNAN_BITS, SNAN_BITS]


def ulp_ladder(c: float, max_pow: int = 12) -> list[float]:
    """c + d fp32 ulps of c for d in 0, +-1, +-2, +-4 ... +-2^max_pow (stepping float by float)."""
    out = [c]
    for k in range(max_pow + 1):
        for sgn in (1, -1):
            x = F32(c)
            for _ in range(1 << k):
                x = np.nextafter(x, F32(sgn * np.inf))
            out.append(float(x))
    return out


def tap_points() -> list[tuple[float, float]]:
    """(cmp, t) pairs: the special texels against ordinary, tiny, large and NaN compare values, and fp32 ulp ladders of the
    texel around each compare value (the straddling pair included: t = pred(cmp) and t = cmp)."""
    cmps = [0.0, -0.0, TINY, -TINY, NORM_MIN, 2.0 ** -110, 2.0 ** -100, -(2.0 ** -100), 0.25, 0.5, 0.7, 1.0, 1.5, 2.0 - 2.0 ** -23,
            2.0, 3.9, 4.0, 5.0, 8.0, 9.5, -0.5, -4.0, -5.0, -9.5, float("nan"), float("inf"), float("-inf")]
    pts = [(c, t) for c in cmps for t in SPECIAL_TEXELS]
    for c in cmps:
        if np.isfinite(c):
            pts += [(c, t) for t in ulp_ladder(c, 6)]
    pts += [(0.5, t) for t in ulp_ladder(0.5, 12)]
    return pts


# ---------------------------------------------------------------------------------------------------------------------
# frames (inputs for the GPU test and the oracle/restatement agreement test)
# ---------------------------------------------------------------------------------------------------------------------
def special_shadow_map(size: int, seed: int) -> np.ndarray:
    """synth.shadow_map_noise with one texel in three replaced by a special value (bits kept: the sNaN stays signalling)."""
    from unclerenderer_amd import synth
    m = np.ascontiguousarray(synth.shadow_map_noise(size, seed), F32).copy()
    bits = m.view(np.uint32)
    rng = np.random.default_rng(seed)
    sel = rng.random(m.shape) < 1 / 3
    specials = np.array(SPECIAL_TEXEL_BITS + [to_bits(v) for v in (4.0, 8.0, 10.0, 1e30, -4.0, -10.0)], np.uint32)
    bits[sel] = specials[rng.integers(0, len(specials), int(sel.sum()))]
    return m


def widen_window(scene, factor: float = 4.0):
    """Scale the light's clip x and y (columns 0 and 1 of LightViewProjection) so that the shadow map covers the middle of the
    frame only: the window's edges and the map's border then cross the frame (the matrix stays orthographic)."""
    for r in range(4):
        for c in (0, 1):
            scene.LightViewProjection[r * 4 + c] = float(F32(scene.LightViewProjection[r * 4 + c] * factor))


def flatten_depth(scene, T: float):
    """Zero the light's depth column and set its constant to T: every pixel's compare value is then exactly T - ShadowBias
    in every evaluation order (kernels, oracle, restatement)."""
    for r in range(3):
        scene.LightViewProjection[r * 4 + 2] = 0.0
    scene.LightViewProjection[14] = T


def exact_cmp_shadow_map(size: int, cmp: float, seed: int) -> np.ndarray:
    """Texels on an fp32 ladder around `cmp` (+-1 .. +-8 ulps, the straddling pair, +-0, +-2^-149, NaN)."""
    vals = [v for v in ulp_ladder(cmp, 3)] + [0.0, -0.0, TINY, -TINY, 2 * TINY, -2 * TINY, f32(QNAN_BITS)]
    rng = np.random.default_rng(seed)
    return np.asarray(vals, F32)[rng.integers(0, len(vals), (size, size))]


def scatter_depths(depth: np.ndarray, seed: int, share: float = 0.25) -> np.ndarray:
    """The stored depth with `share` of its pixels replaced by the special depths (-1, -0, 0, 2^-149, 2, +Inf, qNaN, sNaN)."""
    d = np.ascontiguousarray(depth, F32).copy()
    bits = d.view(np.uint32)
    rng = np.random.default_rng(seed)
    sel = rng.random(d.shape) < share
    bits[sel] = np.asarray(SPECIAL_DEPTH_BITS, np.uint32)[rng.integers(0, len(SPECIAL_DEPTH_BITS), int(sel.sum()))]
    return d


def edge_frame(kind: str, w: int = 320, h: int = 180, seed: int = 7, shadow_size: int = 256, scene_name: str = "sponza"):
    """(fc, g, shadow, exact_cmp) for one edge set:
      texels       the special shadow map, the window widened (border taps with cmp <= 1);
      bias<b>      the same with ShadowBias = b (cmp > 1: border taps fail; |cmp| >= 4: the former gt_step overflowed);
      cmp<T>       depth column zeroed, cmp = T exactly, texels on a ladder around T;
      depth        the stored depth scattered with special values (sky tests).
    exact_cmp: every compare value is exact (no tie can be argued away)."""
    from unclerenderer_amd import hostmath, synth
    fc = hostmath.build_frame_constants(scene_name, w, h, shadow_size=shadow_size, shadow_strength=1.0, env_mip_count=6)
    g = synth.gbuffer_scene(fc.view, fc.proj, fc.camera_position, w, h, seed)
    exact = False
    if kind == "texels" or kind.startswith("bias"):
        widen_window(fc.scene)
        if kind.startswith("bias"):
            fc.scene.ShadowBias = float(kind[4:])
        shadow = special_shadow_map(shadow_size, seed)
    elif kind.startswith("cmp"):
        T = float(F32(float.fromhex(kind[3:])))
        flatten_depth(fc.scene, T)
        fc.scene.ShadowBias = 0.0
        shadow = exact_cmp_shadow_map(shadow_size, T, seed)
        exact = True
    elif kind == "depth":
        g.depth = scatter_depths(g.depth, seed)
        shadow = synth.shadow_map_noise(shadow_size, seed)
    else:
        raise ValueError(kind)
    return fc, g, shadow, exact


EDGE_KINDS = ("texels", "bias-1.5", "bias-4", "bias-8", "bias5", "cmp0x0p+0", "cmp0x1p-130", "cmp0x1p-1", "depth")


def to_bits(x: float) -> int:
    return struct.unpack("<I", struct.pack("<f", x))[0]
