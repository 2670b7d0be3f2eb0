"""The Forward rule restated in numpy: what ur_forward_pass must compute, to the byte.

The front half is tests/gbuffer_mask_ref.py's, called as it is: the opaque raster, the masked raster with its alpha test, the merge that
raises depth, and tests/gbuffer_tex_ref.py's gather of the winning triangle per texel (vertex stage, near clip with its weight rows, the
covering piece, the exact edge values). This file adds the second resolve over those keys: Shaders/ForwardPS.hlsl:73-143 on the
attributes Shaders/ForwardVS.hlsl forms, in two phases as the kernel walks them - material() samples the maps (section 3.10's sampler;
the metallic-roughness map at baseUV, as ForwardPS.hlsl:103 has it) and builds the world normal, light32() does the shadow, EvaluatePBR
and the image-based terms with the fixed-function arithmetic oracle/ur_oracle.cpp's header defines (exact bilinear weights at
uv * size - 0.5, the bordered cube faces, a linear blend of two mips, PCF as a bilinear blend of LESS_EQUAL compares with a white
border, a clamped RG16_UNORM LUT). numpy float32 arithmetic is IEEE, one rounding per operation, no contraction.

With precise=True the same texels are evaluated a second time in float64 from the same fp32 vertex-stage values, integers and texel
codes; the lighting half then is tests/lighting_ref64.py's EnvCube, sample_lut, sample_cmp and evaluate_pbr.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from tests import gbuffer_mask_ref as M
from tests import gbuffer_ref as G
from tests import gbuffer_tex_ref as X
from tests import lighting_ref64 as R

F = np.float32
F64 = np.float64
PLANTS = ("mr_transform", "raw_tangent", "view_normal", "spec0")  # the planted errors of tests/test_forward_ref.py
POISON_HDR = 0x7E5A  # an fp16 NaN: what a test fills `hdr` with where nothing was drawn before

MEASURED_ULPS = 0.5624  # the 257 x 130 soup (0.5487 on 64 x 64): the fp16 store's half ulp and the fp32 error; tests/test_forward_ref.py prints them
ULPS_BOUND = 2.0        # the smallest power of two that is at least twice the measured value


@dataclass
class Frame:
    """The per-frame side of the pass: the fields ur_forward_pass takes from frame_constants, and the lighting tables."""
    camera: np.ndarray
    light_direction: np.ndarray
    light_color: np.ndarray
    light_intensity: float
    lvp: np.ndarray                 # LightViewProjection, 16 floats, row-vector convention
    shadow_strength: float
    shadow_bias: float
    shadow: "np.ndarray | None"     # (H, W) float32; ShadowMapSize = (W, H)
    cube_bits: np.ndarray           # (texels, 4) uint16, DDS order
    env_base: int
    env_mips: int
    lut: np.ndarray                 # (h, w, 2) uint16
    env_mip_count: "float | None" = None  # EnvMapMipCount; None: env_mips
    shadow_size: "tuple | None" = None    # ShadowMapSize when there is no map

    def __post_init__(self):
        self.env = R.EnvCube(self.cube_bits, self.env_base, self.env_mips)
        half = np.ascontiguousarray(self.cube_bits, np.uint16).view(np.float16).astype(F)[:, :3]
        self.bordered = [half[self.env.fold[m]] for m in range(self.env_mips)]  # (6, n + 2, n + 2, 3) per mip: what ur_stage_env_cube writes
        self.lut32 = (np.ascontiguousarray(self.lut, np.uint16).astype(F) / F(65535.0)).astype(F)

    @property
    def size(self):
        if self.shadow is not None:
            return float(self.shadow.shape[1]), float(self.shadow.shape[0])
        return self.shadow_size or (0.0, 0.0)

    @property
    def mip_count(self):
        return float(self.env_mips if self.env_mip_count is None else self.env_mip_count)

    def scene_constants(self):
        """The ur_scene_constants a caller hands to ur_forward_pass: the per-frame fields set, the per-draw ones poisoned with NaN
        (they come from each command's own block)."""
        from unclerenderer_amd import lib
        s = lib.SceneConstants()
        raw = np.frombuffer(s, np.float32)
        raw[:] = np.nan
        s.LightDirection[:] = [float(v) for v in self.light_direction]
        s.LightColor[:] = [float(v) for v in self.light_color]
        s.CameraPosition[:] = [float(v) for v in self.camera]
        s.LightIntensity = float(self.light_intensity)
        s.LightViewProjection[:] = [float(v) for v in np.asarray(self.lvp, F).reshape(-1)]
        s.ShadowStrength, s.ShadowBias = float(self.shadow_strength), float(self.shadow_bias)
        s.ShadowMapSize[:] = self.size
        s.EnvMapMipCount = self.mip_count
        return s


def vertex_tangents(draws, g, T: int, keys_flat) -> np.ndarray:
    """TANGENT.xyz (vertex bytes 32-43) times (float3x3)World of the three vertices of every gathered texel, NOT normalised: (n, 3, 3)."""
    tri = (keys_flat[g["at"]] & np.uint32((1 << T) - 1)).astype(np.int64)
    out = np.zeros((g["at"].size, 3, 3), F)
    for s in np.unique(g["slot"]):
        d = draws[int(s)]
        rows = np.flatnonzero(g["slot"] == s)
        raw = np.ascontiguousarray(d.vertices).reshape(-1).view(np.uint8)
        idx = np.ascontiguousarray(d.indices).reshape(-1).view(np.uint32)
        vi = d.base_vertex + idx[d.start_index + 3 * tri[rows][:, None] + np.arange(3)].astype(np.int64)
        byte = vi.reshape(-1)[:, None] * d.stride + 32 + np.arange(12)
        t = raw[byte].reshape(-1, 12).copy().view(F).reshape(-1, 3, 3)
        W = np.asarray(d.world, F).reshape(4, 4)
        out[rows] = np.stack([(t[:, :, 0] * W[0, k] + t[:, :, 1] * W[1, k]) + t[:, :, 2] * W[2, k] for k in range(3)], axis=2)
    return out


# ---- phase 1: the material -----------------------------------------------------------------------------------------------------------

def material(g, materials, view, ft=np.float32, plant=None):
    """ForwardPS.hlsl:75-106 and ComputeWorldNormal on the gathered texels in `ft` arithmetic: dict of albedo, emissive, n (the world
    normal), wpos (n, 3), metallic, roughness (n,), bits, and info (per map the rows it was sampled on with their N, L and taps)."""
    n = g["at"].size
    cs = g["cs"]
    odd_col, odd_row = (g["px"] & 1) == 1, (g["py"] & 1) == 1
    step_x, step_y = np.where(odd_col, -256, 256)[:, None], np.where(odd_row, -256, 256)[:, None]
    tangents = g["tan"]
    if plant == "raw_tangent":
        tangents = np.concatenate([g["raw_tan"], g["tan"][:, :, 3:4]], axis=2)
    with np.errstate(all="ignore"):
        b = X._weights(g["lam"], g["cw"], g["B"], ft)
        bx = X._weights(g["lam"] + step_x * g["dsx"], g["cw"], g["B"], ft)
        by = X._weights(g["lam"] + step_y * g["dsy"], g["cw"], g["B"], ft)
        nrm, wpos, colour, tan = X._mix(b, g["wn"], ft), X._mix(b, g["wp"], ft), X._mix(b, g["col"], ft), X._mix(b, tangents, ft)
        uvc, uvx, uvy = X._mix(b, g["uv"], ft), X._mix(bx, g["uv"], ft), X._mix(by, g["uv"], ft)
    bits = np.zeros(n, np.int64)
    samples, info = {}, {}
    for name, bit, at in X.MAPS:
        if name == "metallic_roughness" and plant != "mr_transform":
            at = 112  # ForwardPS.hlsl:103: sampled at baseUV
        samples[name] = np.ones((n, 3), ft)
        for s in np.unique(g["slot"]):
            m = materials[int(s)] if int(s) < len(materials) else None
            tex = m.get(name) if m is not None and (int(m.get("key", 0)) & bit) else None
            if tex is None or not tex.valid:
                continue
            rows = np.flatnonzero(g["slot"] == s)
            bits[rows] |= bit
            with np.errstate(all="ignore"):
                c = cs[rows]
                tu, tv = X.transform(c, at, uvc[rows, 0], uvc[rows, 1], ft)
                xu, xv = X.transform(c, at, uvx[rows, 0], uvx[rows, 1], ft)
                yu, yv = X.transform(c, at, uvy[rows, 0], uvy[rows, 1], ft)
                oc, orow = odd_col[rows], odd_row[rows]
                dxu, dxv = np.where(oc, tu - xu, xu - tu), np.where(oc, tv - xv, xv - tv)
                dyu, dyv = np.where(orow, tu - yu, yu - tu), np.where(orow, tv - yv, yv - tv)
            rgb, N, L, taps = X.sample(tex, tu, tv, dxu, dxv, dyu, dyv, ft)
            samples[name][rows] = rgb
            info.setdefault(name, []).append((rows, N, L, taps))
    _sum3, _norm = X._sum3, X._norm
    with np.errstate(all="ignore"):
        vn = _norm(nrm)
        wnrm = vn.copy()
        use = (bits & X.NORMAL) != 0
        if use.any():
            T3, tw = tan[:, :3], tan[:, 3]
            dt = _sum3(vn[:, 0] * T3[:, 0], vn[:, 1] * T3[:, 1], vn[:, 2] * T3[:, 2])
            t = _norm(T3 - vn * dt[:, None])
            c = np.stack([vn[:, 1] * t[:, 2] - vn[:, 2] * t[:, 1], vn[:, 2] * t[:, 0] - vn[:, 0] * t[:, 2], vn[:, 0] * t[:, 1] - vn[:, 1] * t[:, 0]], axis=1)
            bt = _norm(c) * tw[:, None]
            nm = samples["normal"]
            t0, t1, t2 = nm[:, 0] * ft(2.0) - ft(1.0), nm[:, 1] * ft(2.0) - ft(1.0), nm[:, 2] * ft(2.0) - ft(1.0)
            flat = np.sqrt(_sum3(t0 * t0, t1 * t1, t2 * t2)) < ft(F(1e-5))
            e0, e1, e2 = np.where(flat, ft(0.0), t0), np.where(flat, ft(0.0), t1), np.where(flat, ft(1.0), t2)
            wn = np.stack([_sum3(e0 * t[:, k], e1 * bt[:, k], e2 * vn[:, k]) for k in range(3)], axis=1)
            wnrm = np.where(use[:, None], _norm(wn), vn)
        if plant == "view_normal":
            V = np.asarray(view, F).reshape(4, 4).astype(ft)
            wnrm = _norm(np.stack([_sum3(wnrm[:, 0] * V[0, k], wnrm[:, 1] * V[1, k], wnrm[:, 2] * V[2, k]) for k in range(3)], axis=1))
        albedo = cs[:, 64:67].astype(ft) * colour
        albedo = np.where(((bits & X.BASE_COLOR) != 0)[:, None], albedo * samples["base_color"], albedo)
        mr = samples["metallic_roughness"]
        has_mr = (bits & X.METALLIC_ROUGHNESS) != 0
        metallic = np.where(has_mr, cs[:, 104].astype(ft) * mr[:, 2], cs[:, 104].astype(ft))
        roughness = np.where(has_mr, cs[:, 105].astype(ft) * mr[:, 1], cs[:, 105].astype(ft))
        emissive = np.where(((bits & X.EMISSIVE) != 0)[:, None], cs[:, 80:83].astype(ft) * samples["emissive"], cs[:, 80:83].astype(ft))
    return {"albedo": albedo, "emissive": emissive, "n": wnrm, "wpos": wpos, "metallic": metallic, "roughness": roughness, "bits": bits, "info": info}


# ---- phase 2 in fp32: the fixed-function units and the shading ----------------------------------------------------------------------------

def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _sat(x):
    """saturate as the kernel writes it: x < 0 ? 0 : (x > 1 ? 1 : x); a NaN stays."""
    return np.where(x < 0, x.dtype.type(0), np.where(x > 1, x.dtype.type(1), x))


def _at_least(x, c):
    """max(x, c) as the kernel writes it: x < c ? c : x; a NaN stays."""
    return np.where(x < c, c, x)


def _mix2(a, b, t):
    return a + t * (b - a)


def cube_face32(d):
    """(face, u, v) of fp32 directions (n, 3): the major axis with ties z > y > x, u = (sc / |ma| + 1) * 0.5."""
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    ax, ay, az = np.abs(x), np.abs(y), np.abs(z)
    zmaj = (az >= ax) & (az >= ay)
    ymaj = ~zmaj & (ay >= ax)
    comp = np.where(zmaj, z, np.where(ymaj, y, x))
    face = np.where(zmaj, 4, np.where(ymaj, 2, 0)) + (comp < 0)
    ma = np.abs(comp)
    sc = np.choose(face, [-z, z, x, x, x, -x])
    tc = np.choose(face, [-y, -y, z, -z, -y, -y])
    with np.errstate(all="ignore"):
        return face, (sc / ma + F(1.0)) * F(0.5), (tc / ma + F(1.0)) * F(0.5)


def cube_bilinear32(frame: Frame, mip: int, face, u, v):
    n = frame.env.sizes[mip]
    ok = np.isfinite(u) & np.isfinite(v)
    x, y = np.where(ok, u, F(0.5)) * F(n) - F(0.5), np.where(ok, v, F(0.5)) * F(n) - F(0.5)
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = (x - x0)[:, None], (y - y0)[:, None]
    i0, j0 = np.clip(x0.astype(np.int64) + 1, 0, n), np.clip(y0.astype(np.int64) + 1, 0, n)
    tex = frame.bordered[mip]
    top = _mix2(tex[face, j0, i0], tex[face, j0, i0 + 1], fx)
    bottom = _mix2(tex[face, j0 + 1, i0], tex[face, j0 + 1, i0 + 1], fx)
    return np.where(ok[:, None], _mix2(top, bottom, fy), F(np.nan)).astype(F)


def cube_level32(frame: Frame, d, level):
    """TextureCube.SampleLevel in fp32: the level clamped to [0, mips - 1], the two mips around it blended unless the fraction is 0."""
    face, u, v = cube_face32(d)
    top = F(frame.env_mips - 1)
    lv = np.where(level < 0, F(0.0), np.where(level > top, top, level)).astype(F)
    m0 = np.where(np.isnan(lv), 0, np.floor(np.nan_to_num(lv))).astype(np.int64)
    fl = (lv - m0.astype(F)).astype(F)
    out = np.zeros((d.shape[0], 3), F)
    for m in np.unique(m0):
        sel = np.flatnonzero(m0 == m)
        c0 = cube_bilinear32(frame, int(m), face[sel], u[sel], v[sel])
        f = fl[sel][:, None]
        if (f != 0).any():
            c1 = cube_bilinear32(frame, min(int(m) + 1, frame.env_mips - 1), face[sel], u[sel], v[sel])
            with np.errstate(all="ignore"):
                c0 = np.where(f != 0, _mix2(c0, c1, f), c0)
        out[sel] = c0
    return out


def lut32(frame: Frame, u, v):
    H, W = frame.lut32.shape[:2]
    ok = np.isfinite(u) & np.isfinite(v)
    x, y = np.where(ok, u, F(0.0)) * F(W) - F(0.5), np.where(ok, v, F(0.0)) * F(H) - F(0.5)
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = (x - x0)[:, None], (y - y0)[:, None]
    i0, j0 = np.clip(x0, -1, W).astype(np.int64), np.clip(y0, -1, H).astype(np.int64)
    i1, j1 = np.clip(i0 + 1, 0, W - 1), np.clip(j0 + 1, 0, H - 1)
    i0, j0 = np.clip(i0, 0, W - 1), np.clip(j0, 0, H - 1)
    t = frame.lut32
    out = _mix2(_mix2(t[j0, i0], t[j0, i1], fx), _mix2(t[j1, i0], t[j1, i1], fx), fy)
    return np.where(ok[:, None], out, F(np.nan)).astype(F)


def sample_cmp32(shadow, u, v, cmp):
    """SampleCmpLevelZero in fp32: four LESS_EQUAL compares around uv * size - 0.5, border 1.0, blended bilinearly."""
    H, W = shadow.shape
    x, y = u * F(W) - F(0.5), v * F(H) - F(0.5)
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = x - x0, y - y0
    i0, j0 = x0.astype(np.int64), y0.astype(np.int64)
    r = []
    for dj in (0, 1):
        for di in (0, 1):
            i, j = i0 + di, j0 + dj
            inside = (i >= 0) & (j >= 0) & (i < W) & (j < H)
            t = np.where(inside, shadow[np.clip(j, 0, H - 1), np.clip(i, 0, W - 1)], F(1.0))
            r.append((cmp <= t).astype(F))
    return _mix2(_mix2(r[0], r[1], fx), _mix2(r[2], r[3], fx), fy)


def shadow_coordinates(m, frame: Frame, ft):
    """(shadowUV (n, 2), shadowDepth - ShadowBias, the window test) of ForwardPS.hlsl:109-114 in `ft` arithmetic."""
    Mx = np.asarray(frame.lvp, F).reshape(4, 4).astype(ft)
    wp = m["wpos"]
    with np.errstate(all="ignore"):
        sp = [((wp[:, 0] * Mx[0, k] + wp[:, 1] * Mx[1, k]) + wp[:, 2] * Mx[2, k]) + Mx[3, k] for k in range(4)]
        sc = [sp[k] / sp[3] for k in range(3)]
        suv = np.stack([sc[0] * ft(0.5) + ft(0.5), sc[1] * ft(-0.5) + ft(0.5)], axis=1)
        inside = (suv >= 0).all(axis=1) & (suv <= 1).all(axis=1)
        return suv, sc[2] - ft(F(frame.shadow_bias)), inside


def light32(m, frame: Frame, plant=None):
    """ForwardPS.hlsl:97-142 in fp32 on phase 1's values: the colour (n, 3) before the fp16 store."""
    n = m["n"].shape[0]
    albedo, metallic, roughness, N = m["albedo"], m["metallic"], m["roughness"], m["n"]
    with np.errstate(all="ignore"):
        cam = np.asarray(frame.camera, F)
        toeye = cam[None, :] - m["wpos"]
        V = (toeye / np.sqrt(_dot(toeye, toeye))[:, None]).astype(F)
        ld = np.asarray(frame.light_direction, F)
        L = np.broadcast_to((ld / np.sqrt((ld[0] * ld[0] + ld[1] * ld[1]) + ld[2] * ld[2])).astype(F), (n, 3))
        spec0 = F(np.float16(0.04)) if plant == "spec0" else F(0.04)
        F0 = spec0 + metallic[:, None] * (albedo - spec0)
        # ---- the shadow
        shadow = np.ones(n, F)
        if F(frame.shadow_strength) > 0:
            suv, cmpv, inside = shadow_coordinates(m, frame, F)
            rows = np.flatnonzero(inside)
            sw, sh = frame.size
            hx, hy = F(0.5) / F(sw), F(0.5) / F(sh)
            u, v, c = suv[rows, 0], suv[rows, 1], cmpv[rows]
            s = [sample_cmp32(frame.shadow, u + du, v + dv, c) for du, dv in ((hx, hy), (-hx, hy), (hx, -hy), (-hx, -hy))]
            pcf = F(0.25) * (((s[0] + s[1]) + s[2]) + s[3])
            shadow[rows] = F(1.0) + F(frame.shadow_strength) * (pcf - F(1.0))
        # ---- EvaluatePBR (PBRCommon.hlsl)
        hv = V + L
        Hh = hv / np.sqrt(_dot(hv, hv))[:, None]
        NdotL, NdotV, NdotH, VdotH = _sat(_dot(N, L)), _sat(_dot(N, V)), _sat(_dot(N, Hh)), _sat(_dot(V, Hh))
        alpha = roughness * roughness
        alpha2 = alpha * alpha
        denom = (NdotH * NdotH) * (alpha2 - F(1.0)) + F(1.0)
        Dg = alpha2 / _at_least((F(3.14159265) * denom) * denom, F(1e-4))
        k = roughness + F(1.0)
        k = (k * k) / F(8.0)
        Gs = (NdotV / (NdotV * (F(1.0) - k) + k)) * (NdotL / (NdotL * (F(1.0) - k) + k))
        x1 = F(1.0) - VdotH
        x2 = x1 * x1
        p5 = (x2 * x2) * x1
        Fr = F0 + (F(1.0) - F0) * p5[:, None]
        specular = ((Dg * Gs)[:, None] * Fr) / _at_least((F(4.0) * NdotL) * NdotV, F(1e-4))[:, None]
        kd = (F(1.0) - Fr) * (F(1.0) - metallic)[:, None]
        pbr = (kd * albedo + specular) * NdotL[:, None]
        lc = np.asarray(frame.light_color, F)
        lighting = ((pbr * F(frame.light_intensity)) * lc[None, :]) * shadow[:, None]
        # ---- the image-based terms
        inc = -V
        refl = inc - (F(2.0) * _dot(inc, N))[:, None] * N
        mm = F(frame.mip_count) - F(1.0)
        max_mip = mm if mm > 0 else F(0.0)
        pre = cube_level32(frame, refl.astype(F), (roughness * max_mip).astype(F))
        brdf = lut32(frame, NdotV, roughness)
        spec_ibl = pre * (F0 * brdf[:, 0:1] + brdf[:, 1:2])
        irr = cube_level32(frame, N, np.full(n, max_mip, F))
        diff_ibl = (irr * albedo) * (F(1.0) - metallic)[:, None]
        return ((lighting + (diff_ibl + spec_ibl)) + m["emissive"]).astype(F)


# ---- phase 2 in float64 ----------------------------------------------------------------------------------------------------------------

def _face_tie(d):
    a = np.sort(np.abs(d), axis=1)
    with np.errstate(all="ignore"):
        return ~(a[:, 2] - a[:, 1] > R.TIE * a[:, 2])


def light64(m, frame: Frame):
    """The same in float64 with tests/lighting_ref64.py's units: (colour (n, 3), fragile (n,)) - fragile as that file calls it (a PCF
    compare within 1e-5 of flipping, shadowUV within 1e-5 of the window's edge), or a cube-face choice whose two largest |components| are
    within 1e-5 relative."""
    n = m["n"].shape[0]
    albedo, metallic, roughness, N = m["albedo"], m["metallic"], m["roughness"], m["n"]
    with np.errstate(all="ignore"):
        V = R._normalize(np.asarray(frame.camera, F).astype(F64)[None, :] - m["wpos"])
        L = np.broadcast_to(R._normalize(np.asarray(frame.light_direction, F).astype(F64)), (n, 3))
        F0 = R._lerp(R._c(0.04), albedo, metallic[:, None])
        shadow, fragile = np.ones(n, F64), np.zeros(n, bool)
        strength = F64(F(frame.shadow_strength))
        if strength > 0:
            suv, cmpv, inside = shadow_coordinates(m, frame, F64)
            fragile |= np.any((np.abs(suv) <= R.TIE) | (np.abs(suv - 1.0) <= R.TIE), axis=1)
            rows = np.flatnonzero(inside)
            sw, sh = frame.size
            hx, hy = 0.5 / F64(F(sw)), 0.5 / F64(F(sh))
            acc, tie = np.zeros(rows.size), np.zeros(rows.size, bool)
            for du, dv in ((hx, hy), (-hx, hy), (hx, -hy), (-hx, -hy)):
                s, t = R.sample_cmp(frame.shadow, suv[rows, 0] + du, suv[rows, 1] + dv, cmpv[rows])
                acc += s
                tie |= t
            shadow[rows] = R._lerp(1.0, 0.25 * acc, strength)
            fragile[rows] |= tie
        light = np.asarray(frame.light_color, F).astype(F64) * F64(F(frame.light_intensity))
        lighting = R.evaluate_pbr(albedo, metallic, roughness, F0, N, V, L) * light * shadow[:, None]
        inc = -V
        refl = inc - (2.0 * R._dot(N, inc))[:, None] * N
        max_mip = max(0.0, F64(F(frame.mip_count)) - 1.0)
        pre = frame.env.sample_level(refl, roughness * max_mip)
        brdf = R.sample_lut(np.ascontiguousarray(frame.lut, np.uint16), R._sat(R._dot(N, V)), roughness)
        irr = frame.env.sample_level(N, np.full(n, max_mip))
        fragile |= _face_tie(refl) | _face_tie(N)
        ambient = irr * albedo * (1.0 - metallic)[:, None] + pre * (F0 * brdf[:, :1] + brdf[:, 1:])
        return lighting + ambient + m["emissive"], fragile


# ---- the pass ------------------------------------------------------------------------------------------------------------------------------

def forward_pass(draws, view, proj, depth, w: int, h: int, frame: Frame, materials=None, flags: int = 0, select=None, mask_select=None,
                 key_triangle_bits: int = 0, command_count=None, hdr=None, precise: bool = False, plant=None):
    """ur_forward_pass over the whole target (a band is rows of it). mask_select None: mask == NULL (keys are ur_gbuffer_pass_materials',
    depth stays). hdr: the (h, w, 4) uint16 image in front of the pass (None: POISON_HDR everywhere). Returns gbuffer_mask_ref.masked_pass'
    dict with `hdr` the image behind the pass and `color32` (n, 3) the unrounded colour of the gathered texels; precise: `color64`,
    `fragile` and `same` (float64 took the sampler's choices of fp32 on every map of the texel) beside masked_pass' own."""
    out = M.masked_pass(draws, view, proj, depth, w, h, materials=materials, flags=flags, select=select, mask_select=() if mask_select is None else mask_select,
                        key_triangle_bits=key_triangle_bits, command_count=command_count, precise=precise)
    g = out["gather"]
    mats = materials if materials is not None else []
    if plant == "raw_tangent":
        T = G.key_bits(len(draws) if command_count is None else command_count, key_triangle_bits)
        g = dict(g, raw_tan=vertex_tangents(draws, g, T, out["keys"].reshape(-1)))
    m32 = material(g, mats, view, F, plant)
    color = light32(m32, frame, plant)
    image = np.full((h * w, 4), POISON_HDR, np.uint16) if hdr is None else np.ascontiguousarray(hdr, np.uint16).reshape(h * w, 4).copy()
    image[g["at"]] = G._half(np.concatenate([color, np.ones((color.shape[0], 1), F)], axis=1))
    out.update({"hdr": image.reshape(h, w, 4), "color32": color, "material32": m32})
    if precise:
        m64 = material(g, mats, view, F64)
        out["color64"], out["fragile"] = light64(m64, frame)
        same = np.ones(g["at"].size, bool)
        for name, runs in m32["info"].items():
            for (rows, N, L, taps), (_, N64, L64, taps64) in zip(runs, m64["info"][name]):
                same[rows] &= (N == N64) & (L == L64) & (taps == taps64).all(axis=(1, 2, 3))
        out["same"] = same
    return out


def accuracy(out):
    """(the left-out share of the shaded texels, the largest error of a stored channel in fp16 ulps of the float64 value - lighting_ref64's
    measure -) over the texels where float64 takes the same sampler and discard decisions and that lighting_ref64 does not call fragile."""
    at = out["gather"]["at"]
    keep = out["same"] & ~out["fragile"] & ~out["differs"].reshape(-1)[at]
    x = out["color64"]
    bits = out["hdr"].reshape(-1, 4)[at][:, :3]
    with np.errstate(all="ignore"):
        e = np.abs(R.signed_error(bits, x))
    fin = np.isfinite(x) & keep[:, None]
    return float((~keep).sum()) / max(at.size, 1), float(e[fin].max()) if fin.any() else 0.0


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------

SOUPS = M.SOUPS


def soup_frame(w: int, h: int, seed: int) -> Frame:
    """The soups' per-frame side: the eye of depth_ref.soup_camera, a light off every axis, a 64 x 64 shadow map of seeded noise under an
    orthographic light whose window holds the middle of the soup and not its rim, an 8-texel 4-mip cube and the 128 x 32 LUT."""
    from tests import depth_ref as D
    from unclerenderer_amd import synth
    view, _ = D.soup_camera(w, h)
    eye = np.linalg.inv(view.astype(F64).reshape(4, 4))[3, :3].astype(F)
    lvp = np.array([12, -1, 0.2, 0, 1, 12, 0.1, 0, 0.5, 0.5, 3, 0, 7.94, -6.32, 4.224, 1], F)  # (the soup's world positions cluster round (-0.62, 0.5, -1.2))
    return Frame(camera=eye, light_direction=np.array([0.3, 0.8, -0.45], F), light_color=np.array([1.0, 0.95, 0.85], F), light_intensity=3.0, lvp=lvp,
                 shadow_strength=0.75, shadow_bias=0.002, shadow=synth.shadow_map_noise(64, seed), cube_bits=synth.env_cube_procedural(8, 4), env_base=8,
                 env_mips=4, lut=synth.brdf_lut_procedural(128, 32))
