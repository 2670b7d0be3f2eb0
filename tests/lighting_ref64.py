"""Vectorised numpy float64 restatement of DeferredLighting and SkyAtmosphere, written from the HLSL (helper of
tests/test_lighting_ref64.py and tests/test_gpu_accuracy.py; no tests here).

Shaders/DeferredLighting.hlsl:35-94 (PSMain), Shaders/PBRCommon.hlsl:1-48 and Shaders/SkyAtmosphere.hlsl:40-101, with the
arithmetic the hardware leaves open fixed as oracle/ur_oracle.cpp's header defines it:
  * texture filtering with exact weights: a tap at t = uv * size - 0.5 blends the 2x2 texels around it by the fractions of t;
  * seamless cube edges: a tap one texel past a face edge folds onto the adjacent face's texel that touches that edge at the
    same place (the centre of its first texel row, half a texel off the edge); a corner tap clamps the second coordinate first;
  * PCF: the bilinear blend of four LESS_EQUAL compares, an opaque white border (depth 1.0) outside the map;
  * the BRDF LUT: bilinear, clamped, RG16_UNORM texels = value / 65535;
  * sRGB albedo by the formula (c <= 0.04045 ? c / 12.92 : ((c + 0.055) / 1.055)^2.4);
  * the RGBA16F blend: decoded destination plus source;
  * the sky: an analytic sphere of radius World[0] around the camera, depth Projection._43 / z_view.
Every operation runs in float64, so the one rounding left is the fp16 store: the result is the exact value each output
channel should round to. Only the data's own quantisation stays (fp16 G-buffer, depth and cube texels, 8-bit albedo, the
LUT's 16-bit texels, fp32 constants and shadow map).

Discontinuous decisions cannot be settled by an fp32 evaluation when their float64 argument sits on the threshold; such
pixels are returned in `fragile64`: a shadow compare within 1e-5 (relative) of its texel, a shadowUV coordinate within 1e-5
of the [0, 1] window's edge, and a sky depth within 1e-5 (relative) of the stored depth.
"""
from __future__ import annotations

import numpy as np

F64 = np.float64
TIE = 1e-5
CHUNK = 1 << 17  # pixels per vectorised pass: bounds the float64 temporaries


def _c(v) -> F64:
    """A shader literal: the fp32 value the compiled shader holds, widened exactly."""
    return F64(np.float32(v))


PI = _c(3.14159265)


# ---------------------------------------------------------------------------------------------------------------------
# fp16 rounding and the accuracy measures
# ---------------------------------------------------------------------------------------------------------------------
def round16(x: np.ndarray) -> np.ndarray:
    """Round-to-nearest-even to fp16, returned as float64 (float64 -> fp16 directly: one rounding)."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(x, F64).astype(np.float16).astype(F64)


def ulp16(x: np.ndarray) -> np.ndarray:
    """u(x): the fp16 ulp at round16(x) (2^-24 in the subnormal range)."""
    r = np.abs(round16(x))
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.floor(np.log2(np.maximum(np.where(np.isfinite(r), r, 1.0), 2.0 ** -14)))
    return np.exp2(e - 10)


def signed_error(bits: np.ndarray, x: np.ndarray) -> np.ndarray:
    """e = (value - x) / u(x) for RGBA16F bit patterns `bits` against exact values `x` (same shape)."""
    v = np.ascontiguousarray(bits, np.uint16).view(np.float16).astype(F64)
    with np.errstate(invalid="ignore"):
        return (v - x) / ulp16(x)


def measure(bits: np.ndarray, x: np.ndarray, skip: np.ndarray, sky: np.ndarray | None = None) -> dict:
    """Accuracy of the RGBA16F result `bits` against the exact values `x` (both (..., 4)) over the pixels outside `skip` ((...)).
    Returns e (signed errors, NaN where not measured), nan_mismatch (values whose NaN-ness differs from x's), n (finite values
    measured), misround (fraction of them != round16(x)), and the mean of e over the RGB values (mean), over RGB values below
    0.25 (mean_low) and over the RGB values of the `sky` pixels (mean_sky), with their counts n_low and n_sky."""
    x = np.asarray(x, F64)
    v = np.ascontiguousarray(bits, np.uint16).view(np.float16).astype(F64)
    keep = np.broadcast_to(~np.asarray(skip, bool)[..., None], x.shape)
    fin = keep & np.isfinite(x)
    e = np.where(fin, signed_error(bits, x), np.nan)
    rgb = np.zeros(x.shape, bool)
    rgb[..., :3] = True
    low = fin & rgb & (np.abs(x) < 0.25)
    skym = fin & rgb & (np.asarray(sky, bool)[..., None] if sky is not None else False)
    mean = lambda m: float(e[m].mean()) if m.any() else 0.0
    return dict(e=e, nan_mismatch=int((keep & (np.isnan(v) != np.isnan(x))).sum()), n=int(fin.sum()),
                misround=float((v[fin] != round16(x[fin])).mean()) if fin.any() else 0.0,
                mean=mean(fin & rgb), mean_low=mean(low), mean_sky=mean(skym), n_rgb=int((fin & rgb).sum()), n_low=int(low.sum()),
                n_sky=int(skym.sum()))


def r1_violations(e: np.ndarray, e_ref: np.ndarray | None = None) -> np.ndarray:
    """R1 (faithful): |e| <= 1, or |e| <= |e_ref| + 1 where the yardstick `e_ref` is itself farther than one ulp.
    NaN errors (values not measured) never violate."""
    bound = np.ones_like(e) if e_ref is None else np.where(np.abs(e_ref) > 1.0, np.abs(e_ref) + 1.0, 1.0)
    with np.errstate(invalid="ignore"):
        return np.abs(e) > bound


# ---------------------------------------------------------------------------------------------------------------------
# small vector helpers on (..., 3) arrays
# ---------------------------------------------------------------------------------------------------------------------
def _dot(a, b):
    return (a * b).sum(-1)


def _normalize(v):
    with np.errstate(invalid="ignore", divide="ignore"):
        return v / np.sqrt(_dot(v, v))[..., None]


def _sat(x):
    return np.clip(x, 0.0, 1.0)


def _lerp(a, b, t):
    return a + t * (b - a)


def _mat(m) -> np.ndarray:
    """A row_major float4x4 constant: M[i][j] at i * 4 + j; mul(row vector, M)."""
    return np.array(list(m), F64).reshape(4, 4)


def _vec(v) -> np.ndarray:
    return np.array(list(v), F64)


def _pixels(rows, w, pixels):
    if pixels is None:
        y, x = np.meshgrid(np.arange(rows), np.arange(w), indexing="ij")
        return y.ravel(), x.ravel()
    y, x = (np.asarray(p, np.int64).ravel() for p in pixels)
    assert y.shape == x.shape and (y >= 0).all() and (y < rows).all() and (x >= 0).all() and (x < w).all()
    return y, x


def _shape_out(res, rows, w, pixels):
    return res if pixels is not None else res.reshape((rows, w) + res.shape[1:])


def _decode_hdr(hdr, ys, xs):
    if hdr.dtype == np.uint16:
        return np.ascontiguousarray(hdr).view(np.float16)[ys, xs].astype(F64)
    return np.asarray(hdr, F64)[ys, xs]


# ---------------------------------------------------------------------------------------------------------------------
# texture units
# ---------------------------------------------------------------------------------------------------------------------
# Face axes of D3D cube addressing (+X, -X, +Y, -Y, +Z, -Z): direction = normal * ma + uc * U + vc * V with
# u = (uc / ma + 1) / 2, v = (vc / ma + 1) / 2.
_FACE_N = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], F64)
_FACE_U = np.array([[0, 0, -1], [0, 0, 1], [1, 0, 0], [1, 0, 0], [1, 0, 0], [-1, 0, 0]], F64)
_FACE_V = np.array([[0, -1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [0, -1, 0], [0, -1, 0]], F64)


def select_cube_face(d: np.ndarray):
    """(face, u, v) of directions d (..., 3): major axis |z| >= |y| >= |x| on ties; NaN directions give NaN u, v."""
    ax, ay, az = np.abs(d[..., 0]), np.abs(d[..., 1]), np.abs(d[..., 2])
    zmaj = (az >= ax) & (az >= ay)
    ymaj = ~zmaj & (ay >= ax)
    axis = np.where(zmaj, 2, np.where(ymaj, 1, 0))
    comp = np.take_along_axis(d, axis[..., None], -1)[..., 0]
    face = 2 * axis + (comp < 0)  # -0.0 and NaN: positive face
    ma = np.abs(comp)
    with np.errstate(invalid="ignore", divide="ignore"):
        u = (_dot(d, _FACE_U[face]) / ma + 1.0) * 0.5
        v = (_dot(d, _FACE_V[face]) / ma + 1.0) * 0.5
    return face, u, v


class EnvCube:
    """A cube in DDS order (face-major, mips inner), RGBA16F bits (texels, 4), with one fold table per mip that maps the
    bordered tap (face, j + 1, i + 1), i, j in [-1, N], to a texel index."""

    def __init__(self, cube_bits: np.ndarray, base: int, mips: int):
        self.base, self.mips = int(base), int(mips)
        self.texels = np.ascontiguousarray(cube_bits, np.uint16).view(np.float16).astype(F64)[:, :3]
        sizes = [max(1, self.base >> m) for m in range(self.mips)]
        offs = np.concatenate([[0], np.cumsum([n * n for n in sizes])])
        face_stride = int(offs[-1])
        assert self.texels.shape[0] == 6 * face_stride, "cube texel count does not match base / mips"
        self.sizes = sizes
        self.fold = [self._fold_table(n, int(offs[m]), face_stride) for m, n in enumerate(sizes)]

    @staticmethod
    def _fold_table(n, mip_off, face_stride):
        k = np.arange(-1, n + 1)
        j, i = np.meshgrid(k, k, indexing="ij")
        table = np.zeros((6, n + 2, n + 2), np.int64)
        for f in range(6):
            iout, jout = (i < 0) | (i >= n), (j < 0) | (j >= n)
            jj = np.where(iout & jout, np.clip(j, 0, n - 1), j)  # corner: the second coordinate is clamped first
            s, t = 2.0 * (i + 0.5) / n - 1.0, 2.0 * (jj + 0.5) / n - 1.0
            # the overshooting coordinate lands on the adjacent face's plane (+-1) and the face's own axis moves to the
            # centre of the adjacent face's first texel row (half a texel, 1 / n, off the edge); the other coordinate stays
            s_f = np.where(iout, np.sign(s), s)
            t_f = np.where(iout, t, np.where(jout, np.sign(t), t))
            depth = np.where(iout | jout, 1.0 - 1.0 / n, 1.0)
            p = depth[..., None] * _FACE_N[f] + s_f[..., None] * _FACE_U[f] + t_f[..., None] * _FACE_V[f]
            face, u, v = select_cube_face(p)
            ii = np.clip(np.floor(u * n), 0, n - 1).astype(np.int64)
            jj2 = np.clip(np.floor(v * n), 0, n - 1).astype(np.int64)
            table[f] = face * face_stride + mip_off + jj2 * n + ii
        return table

    def bilinear(self, mip, face, u, v):
        n = self.sizes[mip]
        ok = np.isfinite(u) & np.isfinite(v)
        x, y = np.where(ok, u, 0.5) * n - 0.5, np.where(ok, v, 0.5) * n - 0.5
        x0, y0 = np.floor(x), np.floor(y)
        fx, fy = (x - x0)[..., None], (y - y0)[..., None]
        i0 = x0.astype(np.int64) + 1  # bordered index of the left / top tap
        j0 = y0.astype(np.int64) + 1
        tab, tex = self.fold[mip], self.texels
        t00, t10 = tex[tab[face, j0, i0]], tex[tab[face, j0, i0 + 1]]
        t01, t11 = tex[tab[face, j0 + 1, i0]], tex[tab[face, j0 + 1, i0 + 1]]
        out = _lerp(_lerp(t00, t10, fx), _lerp(t01, t11, fx), fy)
        return np.where(ok[..., None], out, np.nan)

    def sample_level(self, d, level):
        """TextureCube.SampleLevel, trilinear: the level clamped to [0, mips - 1], the two mips around it blended."""
        face, u, v = select_cube_face(d)
        lv = np.clip(np.broadcast_to(np.asarray(level, F64), u.shape), 0.0, self.mips - 1.0)
        m0 = np.floor(lv).astype(np.int64)
        out = np.empty(u.shape + (3,), F64)
        for m in np.unique(m0):
            sel = m0 == m
            c0 = self.bilinear(int(m), face[sel], u[sel], v[sel])
            fl = (lv[sel] - m)[..., None]
            if m + 1 < self.mips and (fl > 0).any():
                c0 = np.where(fl > 0, _lerp(c0, self.bilinear(int(m) + 1, face[sel], u[sel], v[sel]), fl), c0)
            out[sel] = c0
        return out


def sample_lut(lut_bits: np.ndarray, u, v):
    """Texture2D.Sample of the RG16_UNORM LUT (h, w, 2): bilinear, clamped."""
    H, W = lut_bits.shape[:2]
    tex = lut_bits.astype(F64) / 65535.0
    ok = np.isfinite(u) & np.isfinite(v)
    x, y = np.where(ok, u, 0.0) * W - 0.5, np.where(ok, v, 0.0) * H - 0.5
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = (x - x0)[..., None], (y - y0)[..., None]
    i0, j0 = x0.astype(np.int64), y0.astype(np.int64)
    i1, j1 = np.clip(i0 + 1, 0, W - 1), np.clip(j0 + 1, 0, H - 1)
    i0, j0 = np.clip(i0, 0, W - 1), np.clip(j0, 0, H - 1)
    out = _lerp(_lerp(tex[j0, i0], tex[j0, i1], fx), _lerp(tex[j1, i0], tex[j1, i1], fx), fy)
    return np.where(ok[..., None], out, np.nan)


def sample_cmp(shadow: np.ndarray, u, v, cmp):
    """SampleCmpLevelZero (LESS_EQUAL, bilinear, opaque white border). Returns (value, tie) where tie marks a compare
    whose two sides are within 1e-5 (relative) of each other."""
    H, W = shadow.shape
    x, y = u * W - 0.5, v * H - 0.5
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = x - x0, y - y0
    i0, j0 = x0.astype(np.int64), y0.astype(np.int64)
    tie = np.zeros(u.shape, bool)
    r = []
    for dj in (0, 1):
        for di in (0, 1):
            i, j = i0 + di, j0 + dj
            inside = (i >= 0) & (j >= 0) & (i < W) & (j < H)
            t = np.where(inside, shadow[np.clip(j, 0, H - 1), np.clip(i, 0, W - 1)].astype(F64), 1.0)
            tie |= np.abs(cmp - t) <= TIE * np.maximum(np.abs(cmp), np.abs(t))
            r.append((cmp <= t).astype(F64))
    return _lerp(_lerp(r[0], r[1], fx), _lerp(r[2], r[3], fx), fy), tie


def shadow_decisions(scene, A, w, h, row0=0, rows=None, pixels=None) -> dict:
    """The float64 arguments of PSMain's shadow decisions per pixel (flat (n,) or (n, k) arrays over `pixels`, or the whole band):
    uv (n, 2) shadowUV; inside (n,) the [0, 1] window test; cmp64 (n,) the compare value shadowDepth - ShadowBias; and the four
    SampleCmpLevelZero taps' 3x3 union: ia, ja (n,) the block's first texel (texel (ia + c, ja + r) for r, c in 0..2) and
    wx, wy (n, 3) its separable weights (1 - f, 1, f) per axis, whose products sum to 4."""
    rows = A.shape[0] if rows is None else rows
    ys, xs = _pixels(rows, w, pixels)
    ViewInverse, Projection, LVP = _mat(scene.ViewInverse), _mat(scene.Projection), _mat(scene.LightViewProjection)
    depth = np.ascontiguousarray(A, np.uint16).view(np.float16)[ys, xs, 3].astype(F64)
    ndcx, ndcy = (xs + 0.5) / w * 2.0 - 1.0, (ys + row0 + 0.5) / h * 2.0 - 1.0
    viewZ = -depth
    viewPos = np.stack([ndcx * viewZ / Projection[0, 0], -ndcy * viewZ / Projection[1, 1], viewZ], -1)
    worldPos = viewPos @ ViewInverse[:3, :3] + ViewInverse[3, :3]
    sp = worldPos @ LVP[:3, :] + LVP[3, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        sc = sp[:, :3] / sp[:, 3:]
    uv = np.stack([sc[:, 0] * 0.5 + 0.5, sc[:, 1] * -0.5 + 0.5], -1)
    x, y = uv[:, 0] * F64(scene.ShadowMapSize[0]) - 0.5, uv[:, 1] * F64(scene.ShadowMapSize[1]) - 0.5
    ok = np.isfinite(x) & np.isfinite(y)
    x0, y0 = np.floor(np.where(ok, x, 0.0)), np.floor(np.where(ok, y, 0.0))
    fx, fy = x - x0, y - y0
    return dict(uv=uv, inside=np.all((uv >= 0.0) & (uv <= 1.0), -1), cmp64=sc[:, 2] - F64(scene.ShadowBias),
                ia=x0.astype(np.int64), ja=y0.astype(np.int64), wx=np.stack([1.0 - fx, np.ones_like(fx), fx], -1),
                wy=np.stack([1.0 - fy, np.ones_like(fy), fy], -1))


def srgb_to_linear(byte) -> np.ndarray:
    c = np.asarray(byte, F64) / 255.0
    return np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)


# ---------------------------------------------------------------------------------------------------------------------
# PBRCommon.hlsl
# ---------------------------------------------------------------------------------------------------------------------
def distribution_ggx(NdotH, alpha):
    alpha2 = alpha * alpha
    denom = (NdotH * NdotH) * (alpha2 - 1.0) + 1.0
    return alpha2 / np.maximum(PI * denom * denom, _c(1e-4))


def geometry_schlick_ggx(NdotX, k):
    with np.errstate(invalid="ignore", divide="ignore"):
        return NdotX / (NdotX * (1.0 - k) + k)


def fresnel_schlick(VdotH, F0):
    return F0 + (1.0 - F0) * ((1.0 - VdotH) ** 5)[..., None]


def evaluate_pbr(albedo, metallic, roughness, F0, N, V, L):
    """PBRCommon.hlsl:EvaluatePBR on (..., 3) vectors and (...) scalars."""
    H = _normalize(V + L)
    NdotL = _sat(_dot(N, L))
    NdotV = _sat(_dot(N, V))
    NdotH = _sat(_dot(N, H))
    VdotH = _sat(_dot(V, H))
    alpha = roughness * roughness
    D = distribution_ggx(NdotH, alpha)
    k = roughness + 1.0
    k = (k * k) / 8.0
    G = geometry_schlick_ggx(NdotV, k) * geometry_schlick_ggx(NdotL, k)
    Fr = fresnel_schlick(VdotH, F0)
    specular = (D * G)[..., None] * Fr / np.maximum(4.0 * NdotL * NdotV, _c(1e-4))[..., None]
    kd = (1.0 - Fr) * (1.0 - metallic)[..., None]
    diffuse = kd * albedo  # "/ PI" is commented out in the reference
    return (diffuse + specular) * NdotL[..., None]


# ---------------------------------------------------------------------------------------------------------------------
# DeferredLighting.hlsl:PSMain
# ---------------------------------------------------------------------------------------------------------------------
def _lighting_chunk(S, a, b, c, px, py, w, h, shadow, env, lut):
    """PSMain for pixels (px, py) of a w x h frame; a, b: (n, 4) decoded G-buffer texels, c: (n,) packed RGBA8.
    Returns (color (n, 3), fragile64 (n,))."""
    View, ViewInverse, Projection, LVP = _mat(S.View), _mat(S.ViewInverse), _mat(S.Projection), _mat(S.LightViewProjection)
    normal = _normalize(a[:, :3])
    depth = a[:, 3]
    albedo = srgb_to_linear(np.stack([c & 0xFF, (c >> 8) & 0xFF, (c >> 16) & 0xFF], -1))
    roughness, metallic = b[:, 2], b[:, 1]
    F0 = _lerp(b[:, :1], albedo, metallic[:, None])

    uvx, uvy = (px + 0.5) / w, (py + 0.5) / h  # the fullscreen triangle's UV at the pixel centre
    ndcx, ndcy = uvx * 2.0 - 1.0, uvy * 2.0 - 1.0
    viewZ = -depth
    viewPos = np.stack([ndcx * viewZ / Projection[0, 0], -ndcy * viewZ / Projection[1, 1], viewZ], -1)

    V = _normalize(-viewPos)
    L = _normalize(_vec(S.LightDirection) @ View[:3, :3])

    worldPos = viewPos @ ViewInverse[:3, :3] + ViewInverse[3, :3]
    shadowPosition = worldPos @ LVP[:3, :] + LVP[3, :]
    shadowCoord = shadowPosition[:, :3] / shadowPosition[:, 3:]
    shadowUV = np.stack([shadowCoord[:, 0] * 0.5 + 0.5, shadowCoord[:, 1] * -0.5 + 0.5], -1)
    shadowDepth = shadowCoord[:, 2]
    shadow_f = np.ones(len(px), F64)
    fragile = np.zeros(len(px), bool)
    strength = F64(S.ShadowStrength)
    if strength > 0.0 and shadow is not None:
        inside = np.all((shadowUV >= 0.0) & (shadowUV <= 1.0), -1)
        fragile |= np.any((np.abs(shadowUV) <= TIE) | (np.abs(shadowUV - 1.0) <= TIE), -1)
        tx, ty = 1.0 / F64(S.ShadowMapSize[0]), 1.0 / F64(S.ShadowMapSize[1])
        cmp = shadowDepth - F64(S.ShadowBias)
        u, v = shadowUV[inside, 0], shadowUV[inside, 1]
        cm = cmp[inside]
        acc, tie = np.zeros(len(u), F64), np.zeros(len(u), bool)
        for du, dv in ((0.0, 0.0), (tx, 0.0), (0.0, ty), (tx, ty)):
            s, t = sample_cmp(shadow, u + du, v + dv, cm)
            acc += s
            tie |= t
        shadow_f[inside] = _lerp(1.0, 0.25 * acc, strength)
        fragile[inside] |= tie

    light = _vec(S.LightColor) * F64(S.LightIntensity)
    lighting = evaluate_pbr(albedo, metallic, roughness, F0, normal, V, L) * light * shadow_f[:, None]

    worldNormal = _normalize(normal @ ViewInverse[:3, :3])
    worldView = _normalize(_vec(S.CameraPosition) - worldPos)
    i = -worldView
    reflection = i - (2.0 * _dot(worldNormal, i))[:, None] * worldNormal

    maxMip = max(0.0, F64(S.EnvMapMipCount) - 1.0)
    prefiltered = env.sample_level(reflection, roughness * maxMip)
    NdotV = _sat(_dot(worldNormal, worldView))
    brdf = sample_lut(lut, NdotV, roughness)
    specularIbl = prefiltered * (F0 * brdf[:, :1] + brdf[:, 1:])
    irradiance = env.sample_level(worldNormal, np.full(len(px), maxMip))
    diffuseIbl = irradiance * albedo * (1.0 - metallic)[:, None]
    return lighting + diffuseIbl + specularIbl, fragile


def deferred_lighting64(scene, A, B, Cc, shadow, env_cube, env_base, env_mips, lut, hdr, w, h, row0=0, rows=None, pixels=None,
                        env: EnvCube | None = None):
    """Same inputs as oracle.deferred_lighting (band-local arrays). Returns (x, fragile64): the exact RGBA values after the
    ONE/ONE blend, (rows, w, 4) float64 and (rows, w) bool; with `pixels` = (y, x) band-local index arrays, (n, 4) and (n,).
    `env` may carry a prebuilt EnvCube of env_cube (its fold tables are reused across calls)."""
    rows = A.shape[0] if rows is None else rows
    env = env if env is not None else EnvCube(env_cube, env_base, env_mips)
    lut = np.ascontiguousarray(lut, np.uint16)
    sh = np.ascontiguousarray(shadow, np.float32) if shadow is not None else None
    ys, xs = _pixels(rows, w, pixels)
    Ah, Bh = np.ascontiguousarray(A, np.uint16).view(np.float16), np.ascontiguousarray(B, np.uint16).view(np.float16)
    Cu = np.ascontiguousarray(Cc, np.uint32)
    x = np.empty((len(ys), 4), F64)
    frag = np.empty(len(ys), bool)
    for k in range(0, len(ys), CHUNK):
        y, xx = ys[k:k + CHUNK], xs[k:k + CHUNK]
        col, fr = _lighting_chunk(scene, Ah[y, xx].astype(F64), Bh[y, xx].astype(F64), Cu[y, xx].astype(np.int64),
                                  xx.astype(F64), (y + row0).astype(F64), w, h, sh, env, lut)
        dst = _decode_hdr(hdr, y, xx)
        x[k:k + CHUNK, :3] = dst[:, :3] + col
        x[k:k + CHUNK, 3] = dst[:, 3] + 1.0
        frag[k:k + CHUNK] = fr
    return _shape_out(x, rows, w, pixels), _shape_out(frag, rows, w, pixels)


# ---------------------------------------------------------------------------------------------------------------------
# SkyAtmosphere.hlsl
# ---------------------------------------------------------------------------------------------------------------------
def rayleigh_phase(cosTheta):
    k = 3.0 / (16.0 * PI)
    return k * (1.0 + cosTheta * cosTheta)


def mie_phase(cosTheta, g):
    g2 = g * g
    denom = (1.0 + g2 - 2.0 * g * cosTheta) ** 1.5
    return (1.0 - g2) / (4.0 * PI * np.maximum(denom, _c(1e-3)))


def apply_atmosphere(sky, viewDir):
    """ApplyAtmosphere on (n, 3) unit directions -> (n, 3)."""
    horizonFalloff = _sat((1.0 - _sat(viewDir[:, 1] * 0.5 + 0.5)) ** 3)
    zenith = np.array([_c(0.05), _c(0.12), _c(0.22)])
    horizon = np.array([_c(0.52), _c(0.68), _c(0.86)])
    baseSky = _lerp(zenith, horizon, horizonFalloff[:, None])
    Ln = _normalize(_vec(sky.LightDirection))
    cosSunView = viewDir @ Ln
    cosSunUp = Ln[1]
    viewHeight = max(0.0, F64(sky.CameraPosition[1]))
    rayleighDensity = np.exp(-viewHeight / 8000.0)
    mieDensity = np.exp(-viewHeight / 1200.0)
    rayleighColor = np.array([_c(0.650), _c(0.570), _c(0.475)])
    scattered = rayleighColor * rayleighDensity * rayleigh_phase(cosSunView)[:, None]
    scattered = scattered + _vec(sky.LightColor) * mieDensity * (mie_phase(cosSunView, _c(0.76)) * _c(0.8))[:, None]
    sunAttenuation = min(max(np.exp(-max(0.0, 1.0 - cosSunUp) * 2.0), 0.0), 1.0)
    return baseSky + scattered * sunAttenuation


def sky_view_dir(sky, px, py, w, h):
    """The camera ray through pixel centres (px, py): view-space (ndc.x / P11, ndc.y / P22, 1) taken to world space by
    View's rotation block transposed. Returns (unit world direction (n, 3), the sphere's depth along the ray (n,))."""
    View, P, World = _mat(sky.View), _mat(sky.Projection), _mat(sky.World)
    uvx, uvy = (px + 0.5) / w, (py + 0.5) / h
    v = np.stack([(uvx * 2.0 - 1.0) / P[0, 0], (1.0 - uvy * 2.0) / P[1, 1], np.ones_like(uvx)], -1)
    world = v @ View[:3, :3].T
    z_view = World[0, 0] * (1.0 / np.sqrt(_dot(v, v)))  # radius * unit_dir.z
    return _normalize(world), P[3, 2] / z_view


def sky_atmosphere64(sky, depth, hdr, w, h, row0=0, rows=None, pixels=None):
    """Same inputs as oracle.sky_atmosphere; `hdr` is the band's RGBA16F bits, or float64 exact values of the same layout as
    the result (e.g. deferred_lighting64's x, gathered at `pixels` when given). Returns (x, fragile64) like
    deferred_lighting64: (sky, 1) where the sphere's depth >= the stored depth, the incoming value elsewhere."""
    depth = np.ascontiguousarray(depth, np.float32)
    rows = depth.shape[0] if rows is None else rows
    ys, xs = _pixels(rows, w, pixels)
    x = np.empty((len(ys), 4), F64)
    frag = np.empty(len(ys), bool)
    flat = pixels is not None and hdr.dtype != np.uint16
    for k in range(0, len(ys), CHUNK):
        y, xx = ys[k:k + CHUNK], xs[k:k + CHUNK]
        d = depth[y, xx].astype(F64)
        dirs, sky_depth = sky_view_dir(sky, xx.astype(F64), (y + row0).astype(F64), w, h)
        draw = sky_depth >= d
        base = np.asarray(hdr, F64)[k:k + CHUNK] if flat else _decode_hdr(hdr, y, xx)
        out = base.copy()
        out[draw, :3] = apply_atmosphere(sky, dirs[draw])
        out[draw, 3] = 1.0
        x[k:k + CHUNK] = out
        frag[k:k + CHUNK] = np.abs(sky_depth - d) <= TIE * np.maximum(np.abs(sky_depth), np.abs(d))
    return _shape_out(x, rows, w, pixels), _shape_out(frag, rows, w, pixels)


def sky_drawn(sky, depth, w, h, row0=0, rows=None, pixels=None):
    """Where the sky pass writes: the sphere's depth >= the stored depth ((rows, w) or (n,) bool)."""
    depth = np.ascontiguousarray(depth, np.float32)
    rows = depth.shape[0] if rows is None else rows
    ys, xs = _pixels(rows, w, pixels)
    _, sky_depth = sky_view_dir(sky, xs.astype(F64), (ys + row0).astype(F64), w, h)
    return _shape_out(sky_depth >= depth[ys, xs], rows, w, pixels)


def n_dot_v(scene, A, w, h, row0=0, rows=None, pixels=None):
    """dot(N, V) of PSMain (view space, unsigned, before saturate): where N is nearly perpendicular to the view ray this
    cosine is a difference of products, and an fp32 evaluation carries an absolute error of ~1e-7 into the terms that scale
    with it (GeometrySchlickGGX(N.V) and, under its 1e-4 clamp, the specular denominator 4 N.L N.V)."""
    rows = A.shape[0] if rows is None else rows
    ys, xs = _pixels(rows, w, pixels)
    Projection = _mat(scene.Projection)
    a = np.ascontiguousarray(A, np.uint16).view(np.float16)[ys, xs].astype(F64)
    uvx, uvy = (xs + 0.5) / w, (ys + row0 + 0.5) / h
    viewZ = -a[:, 3]
    viewPos = np.stack([(uvx * 2.0 - 1.0) * viewZ / Projection[0, 0], -(uvy * 2.0 - 1.0) * viewZ / Projection[1, 1], viewZ], -1)
    return _shape_out(_dot(_normalize(a[:, :3]), _normalize(-viewPos)), rows, w, pixels)


def lighting_sky64(scene, sky, A, B, Cc, depth, shadow, env_cube, env_base, env_mips, lut, hdr, w, h, row0=0, rows=None, pixels=None,
                   env: EnvCube | None = None):
    """Lighting followed by the sky (what the fused launch computes): (x, fragile64) with fragile64 the union of both."""
    lx, lf = deferred_lighting64(scene, A, B, Cc, shadow, env_cube, env_base, env_mips, lut, hdr, w, h, row0, rows, pixels, env)
    sx, sf = sky_atmosphere64(sky, depth, lx, w, h, row0, rows, pixels)
    return sx, lf | sf
