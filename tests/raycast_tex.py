"""The float64 ray caster (tests/raycast_ref.py) carried to the textured, the alpha-masked and the forward pass.

tests/raycast_ref.py finds every hit of every ray; this file interpolates the rest of the 64-byte vertex at a hit with the same
world-space barycentrics (TEXCOORD, the vertex shaders' tangent, COLOR with its alpha), evaluates the pixel shaders in float64 as
Shaders/DeferredBasePass.hlsl and Shaders/ForwardPS.hlsl have them (the comments cite their lines), applies the alpha test to the hits of
the masked draws before a winner is chosen, and shades the forward pass' material with tests/forward_ref.light64. It uses none of the
rule text's formulas: no quad partner, no 8.8 level table, no squared thresholds, no probe offsets - and it never samples a texture.

Textures whose sample does not depend on the filter (Analytic). D3D leaves the anisotropic filter to the implementation, so the scenes
use textures whose correct sample is known without one:
  * "ramp": level k of a 64 x 64 x 4-level UNORM chain holds a_c + bx_c ((i + 0.5) 2^k - 0.5) + by_c ((j + 0.5) 2^k - 0.5) at texel
    (i, j), with bx_c, by_c even so that every code is an integer in [0, 255] at every level. Every level is the same affine function at
    its texel centres; bilinear, trilinear and any symmetric set of probes return (a_c + bx_c (u W - 0.5) + by_c (v H - 0.5)) / 255 as
    long as the footprint stays clear of the wrap seam.
  * "const": one code per channel at every texel of every level (UNORM or _SRGB): checks the decode and the binding, not the uv.
  * "level": level k holds the code 60 k: the sample is 60 (d + f) / 255 whatever uv, taps and probes are, so the level the kernel took
    can be read back from an output as value x 255 / 60.

Which texels are compared: tests/raycast_ref.py's rule (9 rays, one draw, altitude of at least 1 px, one sheet), and further a texel is
left out when
  * its 9 rays do not agree on the sequence of discarded hits (which draws, in which order) in front of the winner;
  * at the centre ray a masked hit at or in front of the winner has |alpha - cutoff| <= the 9-ray spread of that alpha + 2^-16 (alpha is
    a product of three fp32 factors below 2: 2^-16 is over a hundred times its rounding error);
  * the footprint of a sampled ramp reaches the wrap seam: with the one-pixel uv differences below as `major`, u -+ 0.375 |major| or v
    likewise lies within half a texel of the chain's coarsest level of 0 or 1 (a constant or a level-coded map has no seam to reach);
  * a level-coded map's four difference combinations or 9 rays disagree on the probe count N;
  * (forward) the 9 rays disagree on the shadow-window test, on one of the 16 PCF compares or on the cube face of n or of the reflection.
LEFT_OUT_CAP of raycast_ref stays the cap of the share, over the texels any ray hits (a discarded hit counts as one).

Level of detail (level-coded maps only): the rays through the four neighbouring texel centres (x -+ 1, y -+ 1) meet the plane of the ray's
triangle; TEXCOORD is affine on that plane, which gives one-pixel uv differences forwards and backwards in each axis. For each of the four
forward / backward combinations P_x, P_y are the lengths in texels of the two differences, N = min(max(ceil(Pmax / Pmin), 1), 4) and
level = clamp(log2(Pmax / N), 0, mips - 1): D3D's quad-difference convention with the stated anisotropy of 4. The prediction is the mean
of the four levels; its tolerance the spread of the four and of the 9 rays plus 2 / 256.

Tolerances: the ray caster's own 9-ray spread of the value plus the project's bound for that output (gbuffer_tex_ref.A_ULPS_BOUND fp16
ulps for A, B.yz and hdr.rgb, C_CODES_BOUND codes, depth_ref.DEPTH_ERROR_BOUND, forward_ref.ULPS_BOUND fp16 ulps); ObjectId, B.x, B.w, the
alpha channels and covered-or-clear are exact.

Measured margins, restatement against ray caster, largest error / tolerance over the compared texels, 64 x 64 and 257 x 130
(tests/test_raycast_tex.py records them with record_property and asserts each is at most 1). The kernels on an MI355X give the same
figures (tests/test_gpu_raycast_tex.py), and the depth behind ur_depth_prepass there is within 0.0245-0.0295.
  scene            left out         with forward     A                C         B.yz             hdr              other
  textured         1.86 %, 0.28 %   4.39 %, 0.99 %   0.0255, 0.0253   0.2, 0.2  0.0041, 0.0041   0.0041, 0.0040   forward hdr 0.2383, 0.2456
  textured strip   1.15 %, 0.55 %   -                0.0163, 0.0249   0.2, 0.2  0.0045, 0.0047   0.0042, 0.0049
  levels           3.70 %, 2.74 %   -                0.0093, 0.0165   0.2, 0.2  0.4476, 0.4525   0.4436, 0.4526   level hdr 0.4734, 0.4739; level B 0.4732, 0.4746
  masked           1.27 %, 0.28 %   2.69 %, 0.65 %   0.0225, 0.0238   0.2, 0.2  0.0041, 0.0041   0.0040, 0.0040   depth 0.0242, 0.0247; forward hdr 0.2368, 0.2436
A's small ratios are fp16's half ulp over the 128-ulp bound of section 3.10 (the bound is that section's, made for the sampler's fp32
weight error on random textures; a ramp does not show it), C's 0.2 one code over the 4-code bound plus one; the levels' 0.47 is about the 8.8
level's truncation (up to 1 / 256) and the fp16 store over 2 / 256. ObjectId, B.x, B.w, the alpha channels, covered-or-clear, the background's bytes and
`won` agree exactly everywhere. No disagreement between ray caster, restatements and kernels was found, so no rule changed.
"""
from __future__ import annotations

import warnings
from dataclasses import dataclass

import numpy as np

from tests import depth_ref as D
from tests import forward_ref as FW
from tests import gbuffer_mask_ref as M
from tests import gbuffer_tex_ref as X
from tests import raycast_ref as R

ALPHA_MARGIN = 2.0 ** -16
LEVEL_MARGIN = 2.0 / 256.0
HALF_ONE = 0x3C00
NAMES = [name for name, _, _ in X.MAPS]
BIT = {name: bit for name, bit, _ in X.MAPS}


# ---- analytic textures -------------------------------------------------------------------------------------------------------------------

@dataclass
class Analytic:
    """kind "ramp": a, bx, by per channel; "const": a is the code per channel; "level": level k holds 60 k in every channel."""
    kind: str
    a: tuple = (0, 0, 0, 0)
    bx: tuple = (0, 0, 0, 0)
    by: tuple = (0, 0, 0, 0)
    srgb: bool = False
    size: int = 64
    mips: int = 4

    def value(self, u, v, level=None):
        """The float64 sample (n, 4) at the coordinates u, v (n,); a level-coded chain takes the level (n,) instead."""
        n = np.shape(u)[0]
        if self.kind == "level":
            return np.repeat((60.0 * np.asarray(level, np.float64) / 255.0)[:, None], 4, axis=1)
        a = np.asarray(self.a, np.float64)
        if self.kind == "const":
            c = a / 255.0
            if self.srgb:  # the standard sRGB curve; alpha stays linear
                c[:3] = np.where(c[:3] <= 0.04045, c[:3] / 12.92, ((c[:3] + 0.055) / 1.055) ** 2.4)
            return np.broadcast_to(c, (n, 4)).copy()
        x, y = np.asarray(u) * self.size - 0.5, np.asarray(v) * self.size - 0.5
        return (a + x[:, None] * np.asarray(self.bx, np.float64) + y[:, None] * np.asarray(self.by, np.float64)) / 255.0

    def tex(self) -> X.Tex:
        """The chain as the restatement and the kernels take it; every code must be an integer in [0, 255] at every level."""
        assert self.kind in ("ramp", "const", "level") and (self.kind == "const" or not self.srgb)
        assert self.kind == "const" or (self.mips <= 4 and (self.size >> (self.mips - 1)) >= 8)  # the coarsest level is never 1 x 1
        levels = []
        for k in range(self.mips):
            n = self.size >> k
            j, i = np.mgrid[0:n, 0:n]
            if self.kind == "level":
                code = np.full((n, n, 4), 60.0 * k)
            else:
                x, y = (i + 0.5) * 2.0 ** k - 0.5, (j + 0.5) * 2.0 ** k - 0.5
                code = np.asarray(self.a, np.float64) + x[..., None] * np.asarray(self.bx, np.float64) + y[..., None] * np.asarray(self.by, np.float64)
            assert (code == np.round(code)).all() and code.min() >= 0 and code.max() <= 255, (self, k, code.min(), code.max())
            levels.append(code.astype(np.uint8))
        return X.Tex(levels, self.srgb)


def ref_materials(mats):
    """The materials with every Analytic built into a gbuffer_tex_ref.Tex: what the restatements and the device upload take."""
    return [{k: (v.tex() if isinstance(v, Analytic) else v) for k, v in m.items()} for m in mats]


# ---- the shaders' material in float64 ----------------------------------------------------------------------------------------------------

def _f64(a):
    return np.asarray(a, np.float32).astype(np.float64)


def _unit(v):
    with np.errstate(all="ignore"):
        return v / np.linalg.norm(v, axis=-1, keepdims=True)


def transform(d, name, uv):
    """ApplyTextureTransform (DeferredBasePass.hlsl:49-56) with the map's constant vectors as the draw's block holds them (fp32)."""
    off, sc, rot = (getattr(d, "transforms", None) or {}).get(name, ((0, 0), (1, 1), (1, 0)))
    off, sc, rot = _f64(off), _f64(sc), _f64(rot)
    s = uv * sc                                                                                                   # :51
    return np.stack([s[..., 0] * rot[0] - s[..., 1] * rot[1], s[..., 0] * rot[1] + s[..., 1] * rot[0]], axis=-1) + off  # :52-55


def neighbours(H, sel):
    """TEXCOORD (4, n, 2) where the rays one texel to the right, left, below and above of each hit's ray meet the plane of its triangle."""
    w, h = H["w"], H["h"]
    ray = H["ray"][sel]
    k, rest = ray // (h * w), ray % (h * w)
    X0, Y0 = rest % w + 0.5 + R.OFFSETS[k, 0], rest // w + 0.5 + R.OFFSETS[k, 1]
    inv_vp = np.linalg.inv(H["VP"])
    tri = H["tri"][sel]
    A, e1, e2 = H["P"][tri, 0], H["P"][tri, 1] - H["P"][tri, 0], H["P"][tri, 2] - H["P"][tri, 0]
    nrm = np.cross(e1, e2)
    nn = (nrm * nrm).sum(axis=1)
    uv = H["UV"][tri]
    out = []
    for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1)):
        o, d = R._rays(X0 + dx, Y0 + dy, w, h, inv_vp, False)
        with np.errstate(all="ignore"):
            t = ((A - o) * nrm).sum(axis=1) / (d * nrm).sum(axis=1)
            q = o + t[:, None] * d - A
            s1, s2 = (np.cross(q, e2) * nrm).sum(axis=1) / nn, (np.cross(e1, q) * nrm).sum(axis=1) / nn
        out.append(uv[:, 0] + s1[:, None] * (uv[:, 1] - uv[:, 0]) + s2[:, None] * (uv[:, 2] - uv[:, 0]))
    return np.stack(out)


def lod(c, nb, size: int, mips: int):
    """(N (4, n), level (4, n)) of the four forward / backward combinations of the one-pixel differences of the transformed coordinates
    c (n, 2) and nb (4, n, 2) (right, left, below, above)."""
    fx, bx, fy, by = (nb[0] - c) * size, (c - nb[1]) * size, (nb[2] - c) * size, (c - nb[3]) * size
    Ns, Ls = [], []
    with np.errstate(all="ignore"):
        for dx in (fx, bx):
            for dy in (fy, by):
                px, py = np.hypot(dx[:, 0], dx[:, 1]), np.hypot(dy[:, 0], dy[:, 1])
                pmax, pmin = np.maximum(px, py), np.minimum(px, py)
                N = np.clip(np.nan_to_num(np.ceil(pmax / pmin), nan=1.0, posinf=4.0), 1, 4)
                Ns.append(N)
                Ls.append(np.clip(np.log2(pmax / N), 0.0, mips - 1.0))
    return np.stack(Ns), np.stack(Ls)


def evaluate(H, sel, draws, mats, forward: bool = False, only_alpha: bool = False):
    """The pixel shader's material at the hits `sel` (indices into hits()' arrays), in float64: DeferredBasePass.hlsl's PSMain, or with
    `forward` ForwardPS.hlsl's up to line 107. A dict of (n, ..) arrays: albedo, alpha, metallic, roughness, emissive, normal (view space;
    world space with `forward`), wpos, seam, n_disagree, and the level tolerances mr_extra, emissive_extra with level_<map>,
    level_tol_<map> where a level-coded map was sampled."""
    n = sel.size
    b, tri = H["bary"][sel], H["tri"][sel]
    who = H["owner"][tri]
    mix = lambda a: np.einsum("nk,nkc->nc", b, a[tri])  # noqa: E731
    uv, tan, col, nrm = mix(H["UV"]), mix(H["TAN"]), mix(H["C"]), mix(H["N"])
    nb = neighbours(H, sel)
    out = {"albedo": np.zeros((n, 3)), "alpha": np.zeros(n), "metallic": np.zeros(n), "roughness": np.zeros(n), "emissive": np.zeros((n, 3)),
           "normal": np.zeros((n, 3)), "wpos": H["point"][sel], "seam": np.zeros(n, bool), "n_disagree": np.zeros(n, bool),
           "mr_extra": np.zeros(n), "emissive_extra": np.zeros(n)}
    for name in NAMES:
        out["level_" + name], out["level_tol_" + name] = np.full(n, np.nan), np.full(n, np.nan)
    V3 = None if H["V"] is None else H["V"][:3, :3]
    for k in np.unique(who):
        rows = np.flatnonzero(who == k)
        d, m = draws[int(k)], (mats[int(k)] if mats is not None and int(k) < len(mats) else {"key": 0})
        key = int(m.get("key", 0))
        sample = {}
        for name in NAMES:
            if not key & BIT[name] or (only_alpha and name != "base_color"):
                continue
            at = "base_color" if forward and name == "metallic_roughness" else name  # ForwardPS.hlsl:103 samples it at baseUV
            c, cn = transform(d, at, uv[rows]), transform(d, at, nb[:, rows])           # DeferredBasePass.hlsl:108-111, ForwardPS.hlsl:75-77
            tex, level = m[name], None
            if tex.kind == "level":
                N4, L4 = lod(c, cn, tex.size, tex.mips)
                level = L4.mean(axis=0)
                out["n_disagree"][rows] |= (N4 != N4[0]).any(axis=0)
                out["level_" + name][rows], out["level_tol_" + name][rows] = level, L4.max(axis=0) - L4.min(axis=0)
                out["N_" + name] = out.get("N_" + name, np.zeros(n))
                out["N_" + name][rows] = N4[0]
            elif tex.kind == "ramp":
                major = np.abs(cn - c[None]).max(axis=0)
                edge = 0.5 / (tex.size >> (tex.mips - 1))
                out["seam"][rows] |= ((c - 0.375 * major < edge) | (c + 0.375 * major > 1.0 - edge)).any(axis=1)
            sample[name] = tex.value(c[:, 0], c[:, 1], level)
        albedo, alpha = _f64(d.base_color) * col[rows, :3], float(np.float32(getattr(d, "alpha", 1.0))) * col[rows, 3]  # :115-116
        if "base_color" in sample:
            albedo, alpha = albedo * sample["base_color"][:, :3], alpha * sample["base_color"][:, 3]          # :118-120
        out["albedo"][rows], out["alpha"][rows] = albedo, alpha
        if only_alpha:
            continue
        metallic, roughness = np.full(rows.size, float(np.float32(d.metallic))), np.full(rows.size, float(np.float32(d.roughness)))  # :133-134
        if "metallic_roughness" in sample:
            metallic, roughness = metallic * sample["metallic_roughness"][:, 2], roughness * sample["metallic_roughness"][:, 1]     # :136-138 (.bg)
            if m["metallic_roughness"].kind == "level":
                out["mr_extra"][rows] = max(abs(float(d.metallic)), abs(float(d.roughness))) * 60.0 / 255.0 * (out["level_tol_metallic_roughness"][rows] + LEVEL_MARGIN)
        emissive = np.broadcast_to(_f64(d.emissive), (rows.size, 3))                                              # :144
        if "emissive" in sample:
            emissive = emissive * sample["emissive"][:, :3]                                                       # :146
            if m["emissive"].kind == "level":
                out["emissive_extra"][rows] = np.abs(_f64(d.emissive)).max() * 60.0 / 255.0 * (out["level_tol_emissive"][rows] + LEVEL_MARGIN)
        out["metallic"][rows], out["roughness"][rows], out["emissive"][rows] = metallic, roughness, emissive
        vn = _unit(nrm[rows])                                                                                     # :82
        wn = vn
        if "normal" in sample:
            T3, tw = tan[rows, :3], tan[rows, 3]
            t = _unit(T3 - vn * (vn * T3).sum(axis=1, keepdims=True))                                             # :85
            bt = _unit(np.cross(vn, t)) * tw[:, None]                                                             # :86
            if forward:
                tn = sample["normal"][:, :3] * 2.0 - 1.0                                                          # ForwardPS.hlsl:59
            else:
                rg = sample["normal"][:, :2] * 2.0 - 1.0                                                          # :88
                tn = np.concatenate([rg, np.sqrt(np.clip(1.0 - (rg * rg).sum(axis=1), 0.0, 1.0))[:, None]], axis=1)  # :89-90
            tn = np.where((np.linalg.norm(tn, axis=1) < 1e-5)[:, None], [0.0, 0.0, 1.0], tn)                      # :91-93
            wn = _unit(tn[:, 0:1] * t + tn[:, 1:2] * bt + tn[:, 2:3] * vn)                                        # :95-96, the rows of TBN
        out["normal"][rows] = wn if forward else _unit(wn @ V3)                                                   # :98 / :100; ForwardPS.hlsl:67 / :69
    return out


# ---- the cast ----------------------------------------------------------------------------------------------------------------------------

MATERIAL_KEYS = ("albedo", "alpha", "metallic", "roughness", "emissive", "normal", "seam", "n_disagree", "mr_extra", "emissive_extra")


def cast(draws, w: int, h: int, view, proj, mats, masked=(), tile: int = 16):
    """raycast_ref.cast's dict under the camera with the alpha test applied to the hits of the draws `masked` (slots whose material has
    bit 4), the winner's base-pass material in place of `normal` and `albedo`, and: metallic, roughness, emissive, alpha; fnormal,
    fmetallic, froughness, wpos (the forward pass' material); discards (per ray the discarded hits in front of the winner), signature
    (those hits' draws in order), alpha_margin (.., K: alpha - cutoff of the k-th hit at or in front of the winner, NaN if it is not
    masked), touched (any hit at all), seam, n_disagree, and the level records of evaluate()."""
    H = R.hits(draws, w, h, view, proj, tile=tile)
    n, rays = H["ray"].size, 9 * h * w
    who = H["owner"][H["tri"]]
    has_bit = np.array([bool(int((mats[k] if k < len(mats) else {}).get("key", 0)) & M.ALPHA_MASK) and k in set(masked) for k in range(len(draws))], bool)
    is_masked = has_bit[who] if n else np.zeros(0, bool)
    margin = np.full(n, np.nan)
    idx = np.flatnonzero(is_masked)
    if idx.size:
        cutoff = np.array([float(np.float32(getattr(d, "cutoff", 0.0))) for d in draws])
        margin[idx] = evaluate(H, idx, draws, mats, only_alpha=True)["alpha"] - cutoff[who[idx]]
    discard = is_masked & (margin < 0)                                                       # DeferredBasePass.hlsl:123-126
    order = np.lexsort((-H["z"], H["ray"]))
    ray_s = H["ray"][order]
    start = np.r_[True, ray_s[1:] != ray_s[:-1]] if n else np.zeros(0, bool)
    rank = np.arange(n) - np.maximum.accumulate(np.where(start, np.arange(n), 0)) if n else np.zeros(0, np.int64)
    kept = ~discard[order]
    win_rank = np.full(rays, np.iinfo(np.int64).max)
    np.minimum.at(win_rank, ray_s[kept], rank[kept])
    rc = R.winners(H, order[kept & (rank == win_rank[ray_s])])
    front = rank <= win_rank[ray_s]
    gone = front & ~kept
    assert not rank.size or rank[front].max() < 15
    signature = np.zeros(rays, np.int64)
    np.add.at(signature, ray_s[gone], (who[order][gone] + 1) << (4 * rank[gone]))
    K = int(rank[front & is_masked[order]].max()) + 1 if (front & is_masked[order]).any() else 1
    am = np.full((rays, K), np.nan)
    sel = front & is_masked[order]
    am[ray_s[sel], rank[sel]] = margin[order][sel]
    shape = (9, h, w)
    rc["discards"] = np.bincount(ray_s[gone], minlength=rays).reshape(shape)
    rc["signature"], rc["alpha_margin"] = signature.reshape(shape), am.reshape(shape + (K,))
    rc["touched"] = (np.bincount(H["ray"], minlength=rays) > 0).reshape(shape)
    at = np.flatnonzero(rc["index"].reshape(-1) >= 0)
    won = rc["index"].reshape(-1)[at]

    def spread_out(name, values, fill=np.nan):
        full = np.full((rays,) + values.shape[1:], fill, values.dtype)
        full[at] = values
        rc[name] = full.reshape(shape + values.shape[1:])

    base = evaluate(H, won, draws, mats)
    for k, v in base.items():
        if k != "wpos":
            spread_out(k, v, False if v.dtype == bool else np.nan)
    fwd = evaluate(H, won, draws, mats, forward=True)
    for k in ("normal", "metallic", "roughness"):
        spread_out("f" + k, fwd[k])
    spread_out("wpos", fwd["wpos"])
    return rc


def classify(rc, forward: bool = False):
    """(compared (h, w) bool, any_hit (h, w) bool, left-out share): raycast_ref.classify and the rules of the module docstring."""
    compared, any_hit, _ = R.classify(rc)
    same_sequence = (rc["signature"] == rc["signature"][0]).all(axis=0)
    am = rc["alpha_margin"]
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # (an all-NaN column: no masked hit at that place)
        spread = np.nanmax(am, axis=0) - np.nanmin(am, axis=0)
        close = (np.abs(am[0]) <= np.nan_to_num(spread, nan=np.inf) + ALPHA_MARGIN).any(axis=-1)
    compared = compared & same_sequence & ~close & ~rc["seam"].any(axis=0) & ~rc["n_disagree"].any(axis=0)
    if forward:
        compared &= (rc["decisions"] == rc["decisions"][0]).all(axis=0)
    any_hit = any_hit | rc["touched"].any(axis=0)
    return compared, any_hit, float((any_hit & ~compared).sum()) / max(int(any_hit.sum()), 1)


# ---- the forward pass' shading -------------------------------------------------------------------------------------------------------------

def shade_forward(rc, frame: FW.Frame):
    """Adds `color` (9, h, w, 3), forward_ref.light64 of the ray caster's material, and `decisions`: per ray the shadow-window test, the
    16 PCF compares and the cube faces of n and of the reflection, packed into one integer."""
    shape = rc["hit"].shape
    at = np.flatnonzero(rc["hit"].reshape(-1))
    flat = lambda k: rc[k].reshape((-1,) + rc[k].shape[3:])[at]  # noqa: E731
    m = {"albedo": flat("albedo"), "metallic": flat("fmetallic"), "roughness": flat("froughness"), "n": flat("fnormal"), "wpos": flat("wpos"),
         "emissive": flat("emissive")}
    color, _ = FW.light64(m, frame)
    code = np.zeros(at.size, np.int64)
    with np.errstate(all="ignore"):
        if np.float32(frame.shadow_strength) > 0:                                              # ForwardPS.hlsl:114
            suv, cmpv, inside = FW.shadow_coordinates(m, frame, np.float64)                    # :109-112
            code |= inside.astype(np.int64)
            sh = np.asarray(frame.shadow, np.float64)
            sh_h, sh_w = sh.shape
            bit = 1
            for du, dv in ((0.5, 0.5), (-0.5, 0.5), (0.5, -0.5), (-0.5, -0.5)):                # :116-122
                i0 = np.floor(np.nan_to_num((suv[:, 0] + du / sh_w) * sh_w - 0.5)).astype(np.int64)
                j0 = np.floor(np.nan_to_num((suv[:, 1] + dv / sh_h) * sh_h - 0.5)).astype(np.int64)
                for dj in (0, 1):
                    for di in (0, 1):
                        i, j = i0 + di, j0 + dj
                        ok = (i >= 0) & (j >= 0) & (i < sh_w) & (j < sh_h)
                        t = np.where(ok, sh[np.clip(j, 0, sh_h - 1), np.clip(i, 0, sh_w - 1)], 1.0)
                        code |= (inside & (cmpv <= t)).astype(np.int64) << bit
                        bit += 1
        v = _unit(_f64(frame.camera)[None, :] - m["wpos"])                                     # :97
        refl = -v - 2.0 * ((-v) * m["n"]).sum(axis=1, keepdims=True) * m["n"]                  # :128
        code |= FW.cube_face32(m["n"])[0].astype(np.int64) << 20
        code |= FW.cube_face32(refl)[0].astype(np.int64) << 24
    full = np.full((rc["hit"].size, 3), np.nan)
    full[at] = color
    rc["color"] = full.reshape(shape + (3,))
    dec = np.full(rc["hit"].size, -1, np.int64)
    dec[at] = code
    rc["decisions"] = dec.reshape(shape)
    return rc


# ---- comparisons ---------------------------------------------------------------------------------------------------------------------------

def _half_bits(v):
    return np.asarray(v, np.float32).astype(np.float16).view(np.uint16)


def _halves(a):
    return np.asarray(a, np.uint16).view(np.float16).astype(np.float64)


def compare_gbuffer(rc, out, draws, compared=None):
    """A textured G-buffer (gbuffer_tex_ref.gbuffer_pass', gbuffer_mask_ref.masked_pass' or a kernel's dict) against the cast: {output:
    (failures, largest error / tolerance)}; the exact outputs report 0 or inf."""
    compared = classify(rc)[0] if compared is None else compared
    hit, miss = rc["hit"][0] & compared, ~rc["hit"][0] & compared
    who = np.maximum(rc["draw"][0], 0)
    res = {}

    def exact(name, bad):
        bad = bad & compared
        res[name] = (int(bad.sum()), np.inf if bad.any() else 0.0)

    def close(name, got, ref, ulps, extra=None):
        tol = R._spread(ref) + ulps * R.fp16_ulp(ref[0]) + (0.0 if extra is None else extra)
        res[name] = R._fraction(np.abs(got - ref[0]), tol, hit[..., None] & np.ones(got.shape[-1], bool))

    clear = (out["A"] != R.CLEAR_HALF).any(axis=-1) | (out["B"] != R.CLEAR_HALF).any(axis=-1) | (out["hdr"] != R.CLEAR_HALF).any(axis=-1) | (out["C"] != 0xFF000000)
    exact("covered", (miss & clear) | (hit & (out["B"][..., 0] == 0)))
    exact("B.xw", hit & ((out["B"][..., 0] != _half_bits(0.04)) | (out["B"][..., 3] != HALF_ONE)))
    exact("hdr.a", hit & (out["hdr"][..., 3] != HALF_ONE))
    if "object_id" in out:
        want = np.where(rc["hit"][0], np.array([d.object_id for d in draws], np.uint32)[who], 0)
        exact("object_id", out["object_id"] != want)
    with np.errstate(all="ignore"):
        close("A", _halves(out["A"]), np.concatenate([rc["normal"], rc["view_depth"][..., None]], axis=-1), X.A_ULPS_BOUND)
        close("B.yz", _halves(out["B"])[..., 1:3], np.stack([rc["metallic"], rc["roughness"]], axis=-1), X.A_ULPS_BOUND, rc["mr_extra"].max(axis=0)[..., None])
        close("hdr", _halves(out["hdr"])[..., :3], rc["emissive"], X.A_ULPS_BOUND, rc["emissive_extra"].max(axis=0)[..., None])
        code = np.stack([(out["C"] >> s) & 0xFF for s in (0, 8, 16)], axis=-1).astype(np.int64)
        lo, hi = R.srgb8(np.min(rc["albedo"], axis=0)), R.srgb8(np.max(rc["albedo"], axis=0))
        fails, worst = R._fraction(np.abs(code - R.srgb8(rc["albedo"][0])).astype(np.float64), (hi - lo + X.C_CODES_BOUND).astype(np.float64),
                                   hit[..., None] & np.ones(3, bool))
        alpha = hit & ((out["C"] >> 24) != 0xFF)
        res["C"] = (fails + int(alpha.sum()), np.inf if alpha.any() else worst)
    return res


def compare_depth(rc, depth, compared, clear: float = 0.0):
    """The depth behind a pass against the winner's z / w: raycast_ref.compare_depth over this file's compared texels."""
    t = np.asarray(depth, np.float64)
    hit, miss = rc["hit"][0] & compared, ~rc["hit"][0] & compared
    wrong = (miss & (t != clear)) | (hit & (t == clear))
    fails, worst = R._fraction(np.abs(t - rc["depth"][0]), R._spread(rc["depth"]) + D.DEPTH_ERROR_BOUND, hit & ~wrong)
    return {"depth covered": (int(wrong.sum()), np.inf if wrong.any() else 0.0), "depth": (fails, worst)}


def compare_masked(rc, out, draws, masked, compared=None):
    """ur_gbuffer_pass_masked's outputs: the G-buffer, the depth behind the pass and `won`."""
    compared = classify(rc)[0] if compared is None else compared
    res = compare_gbuffer(rc, out, draws, compared)
    res.update(compare_depth(rc, out["depth"], compared))
    least = int((compared & rc["hit"][0] & np.isin(rc["draw"][0], list(masked))).sum())
    most = least + int((~compared).sum())
    bad = not least <= int(out["won"]) <= most
    res["won"] = (int(bad), np.inf if bad else 0.0)
    return res


def compare_forward(rc, hdr, background, compared=None):
    """ur_forward_pass' HDR image against light64 of the ray caster's material; a texel no surviving hit covers keeps the background."""
    compared = classify(rc, forward=True)[0] if compared is None else compared
    hit, miss = rc["hit"][0] & compared, ~rc["hit"][0] & compared
    res = {}
    bad = miss & differs_half(hdr, background).any(axis=-1)
    res["background"] = (int(bad.sum()), np.inf if bad.any() else 0.0)
    bad = hit & (hdr[..., 3] != HALF_ONE)
    res["hdr.a"] = (int(bad.sum()), np.inf if bad.any() else 0.0)
    with np.errstate(all="ignore"):
        ref = rc["color"]
        res["hdr"] = R._fraction(np.abs(_halves(hdr)[..., :3] - ref[0]), R._spread(ref) + FW.ULPS_BOUND * R.fp16_ulp(ref[0]), hit[..., None] & np.ones(3, bool))
    return res


def differs_half(got, want):
    """Where two RGBA16F images differ, NaN compared by NaN-ness."""
    gn, en = np.isnan(np.asarray(got, np.uint16).view(np.float16)), np.isnan(np.asarray(want, np.uint16).view(np.float16))
    return (gn != en) | (~gn & (got != want))


def compare_levels(rc, out, compared=None):
    """The level read back from hdr.r (the emissive map) and from B.y (the metallic-roughness map's .b) against the prediction: {"level
    hdr": .., "level B": ..}; the tolerance is the spread of the four combinations and of the 9 rays plus 2 / 256."""
    compared = classify(rc)[0] if compared is None else compared
    hit = rc["hit"][0] & compared
    res = {}
    with np.errstate(all="ignore"):
        for what, name, got in (("level hdr", "emissive", _halves(out["hdr"])[..., 0]), ("level B", "metallic_roughness", _halves(out["B"])[..., 1])):
            want, tol4 = rc["level_" + name], rc["level_tol_" + name]
            mask = hit & np.isfinite(want[0])
            res[what] = R._fraction(np.abs(got * 255.0 / 60.0 - want[0]), R._spread(want) + tol4.max(axis=0) + LEVEL_MARGIN, mask)
    return res


# ---- scenes --------------------------------------------------------------------------------------------------------------------------------

@dataclass
class Scene:
    name: str
    draws: list
    mats: list
    view: np.ndarray
    proj: np.ndarray
    masked: tuple = ()
    eye: tuple = (0.0, 0.0, 0.0)

    @property
    def opaque(self):
        return [k for k in range(len(self.draws)) if k not in self.masked]


BASE = Analytic("ramp", a=(1, 127, 127, 253), bx=(2, 2, -2, -2), by=(2, -2, 2, -2))
MASK_BASE = Analytic("ramp", a=(1, 127, 127, 1), bx=(2, 2, -2, 4), by=(2, -2, 2, 0))       # alpha rises with u: 49 / 255 at u = 0.2, 205 / 255 at 0.8
METAL_ROUGH = Analytic("ramp", a=(0, 127, 1, 255), bx=(0, -2, 4, 0), by=(0, 2, 0, 0))      # roughness (.g) and metallic (.b) differ everywhere
NORMAL = Analytic("ramp", a=(64, 64, 250, 255), bx=(2, 0, -2, 0), by=(0, 2, 0, 0))         # r, g in [-0.5, 0.5]; b is not the reconstructed z
EMISSIVE = Analytic("ramp", a=(253, 1, 127, 255), bx=(-4, 0, 2, 0), by=(0, 4, -2, 0))
SRGB_CONST = Analytic("const", a=(200, 120, 60, 255), srgb=True)
LEVELS = Analytic("level")
RAMPS = {"base_color": BASE, "metallic_roughness": METAL_ROUGH, "normal": NORMAL, "emissive": EMISSIVE}


def about_centre(scale=(1.0, 1.0), degrees: float = 0.0, shift=(0.0, 0.0)):
    """A texture transform (offset, scale, (cos, sin)) that scales and rotates about (0.5, 0.5) and then shifts."""
    c, s = np.cos(np.radians(degrees)), np.sin(np.radians(degrees))
    x, y = 0.5 * scale[0], 0.5 * scale[1]
    return (0.5 + shift[0] - (x * c - y * s), 0.5 + shift[1] - (x * s + y * c)), tuple(scale), (c, s)


TRANSFORMS_A = {"base_color": about_centre((1.0, 1.0), 25.0), "metallic_roughness": about_centre((1.2, 0.7)),
                "normal": about_centre((0.9, 0.9), -40.0), "emissive": about_centre((0.8, 1.1), 10.0, (0.05, -0.03))}
TRANSFORMS_B = {"base_color": about_centre((0.7, 1.15), -15.0), "metallic_roughness": about_centre((1.0, 1.0), 60.0, (-0.04, 0.02)),
                "normal": about_centre((1.1, 0.8), 33.0), "emissive": about_centre((1.2, 1.2))}


def textured_copy(d, axes, tangent, tangent_w: float, transforms, vertex_alpha=None, cls=X.TexDraw, **kw):
    """A raycast_ref draw with the rest of its vertex filled: TEXCOORD a planar map of the object-space position's coordinates `axes`
    into [0.3, 0.7]^2, TANGENT a smooth field round `tangent` (not normalised, not parallel to the normal but at isolated points) with the
    given w, COLOR.a from alpha(positions) (default 1)."""
    v = np.ascontiguousarray(d.vertices).view(np.float32).reshape(-1, 16).copy()
    pos = v[:, 0:3].astype(np.float64)
    p = pos[:, list(axes)]
    v[:, 6:8] = 0.3 + 0.4 * (p - p.min(axis=0)) / (p.max(axis=0) - p.min(axis=0))
    v[:, 8:11] = np.asarray(tangent, np.float64) + 0.3 * np.stack([np.sin(2.1 * pos[:, 0] + 0.3), np.cos(1.7 * pos[:, 1]), np.sin(1.3 * pos[:, 2])], axis=1)
    v[:, 11] = tangent_w
    v[:, 15] = 1.0 if vertex_alpha is None else vertex_alpha(pos)
    return cls(v.reshape(-1).view(np.uint8).copy(), d.indices, d.world, base_color=d.base_color, emissive=d.emissive, metallic=d.metallic,
               roughness=d.roughness, object_id=d.object_id, transforms=transforms, **kw)


def _material(key, **other):
    m = {"key": key, **RAMPS}
    m.update(other)
    return m


def quad_grid(xs, ys, z, seed: int, **kw):
    """A grid of quads over the given x and y at the depth z(x, y), facing the camera of the mesh scenes, with smooth normals and seeded
    colours: a GDraw in world space."""
    pos = np.array([[x, y, z(x, y)] for y in ys for x in xs])
    nx, ny = len(xs), len(ys)
    faces = []
    for j in range(ny - 1):
        for i in range(nx - 1):
            a = j * nx + i
            faces += [(a, a + 1, a + nx + 1), (a, a + nx + 1, a + nx)]
    nrm = np.array([[0.2 * np.sin(x), 0.2 * np.cos(y), -1.0] for y in ys for x in xs])
    col = np.random.default_rng(seed).uniform(0.2, 1.0, pos.shape)
    return R._gdraw(pos, nrm, col, R._outward_front(pos, faces, np.asarray(R.CAMERA_EYE) - pos), R._world(np.eye(3), (1, 1, 1), (0, 0, 0)), **kw)


def textured_scene(w, h):
    """The torus and the icosphere through each other in front of a wall of quads that spans more than the view: keys 15, 5 and 10, so
    every map occurs with and without its bit; an _SRGB constant base colour on the torus, UNORM ramps elsewhere; TANGENT.w = -1 on the
    icosphere."""
    view, proj = R._camera(R.CAMERA_EYE, R.CAMERA_DIR, w, h)
    wall = quad_grid(np.linspace(-9.0, 8.0, 4), np.linspace(-6.0, 5.0, 4), lambda x, y: 6.5 + 0.1 * x - 0.08 * y, 5, base_color=np.array([0.7, 0.9, 0.6], np.float32),
                     emissive=np.array([0.75, 0.5, 1.5], np.float32), metallic=0.875, roughness=0.625, object_id=9)
    draws = [textured_copy(R.icosphere_draw(translation=(0.1, 0.0, 3.3)), (0, 1), (1.0, 0.2, 0.1), -1.0, TRANSFORMS_A),
             textured_copy(R.torus_draw(), (0, 2), (0.2, 1.0, 0.3), 1.0, TRANSFORMS_B),
             textured_copy(wall, (0, 1), (0.1, 1.0, 0.3), 1.0, TRANSFORMS_A)]
    return Scene("textured", draws, [_material(15), _material(5, base_color=SRGB_CONST), _material(10)], view, proj, eye=R.CAMERA_EYE)


def _strip_draws(w, h, transforms=(TRANSFORMS_A, TRANSFORMS_B), **kw):
    sc = R.strip_scene(w, h)
    strip = textured_copy(sc.draws[0], (0, 2), (1.0, 0.1, 0.2), -1.0, transforms[0], **kw)
    floor = textured_copy(sc.draws[1], (0, 2), (0.3, 0.1, 1.0), 1.0, transforms[1], **kw)
    return sc, [strip, floor]


def textured_strip_scene(w, h):
    """The near-plane strip and the floor with ramps on all four maps: uv and tangent through the near clip and the large-triangle queue."""
    sc, draws = _strip_draws(w, h)
    return Scene("textured strip", draws, [_material(15), _material(15)], sc.view, sc.proj)


LEVEL_TRANSFORMS = ({"emissive": ((0.1, 0.2), (3.0, 40.0), (1.0, 0.0)), "metallic_roughness": ((0.0, 0.0), (1.5, 90.0), (np.cos(0.3), np.sin(0.3)))},
                    {"emissive": ((0.3, 0.1), (100.0, 1.0), (1.0, 0.0)), "metallic_roughness": ((0.0, 0.5), (25.0, 40.0), (np.cos(-0.5), np.sin(-0.5)))})


def levels_scene(w, h):
    """The strip scene's floor and strip with a level-coded emissive map (EmissiveFactor 1) and a level-coded metallic-roughness map
    (both factors 1); the uv scales are chosen so that the compared texels span levels 0 to 3 and every N from 2 to 4. A change of N
    costs the texels along it (forward and backward differences disagree there), and one that runs along a row of the floor costs the
    whole row: two of those alone exceed the cap at 64 x 64. The floor's emissive map therefore has almost no scale in v: its footprint
    is the change of u alone, whose ratio varies across the floor, and N changes along short curves."""
    sc, draws = _strip_draws(w, h, LEVEL_TRANSFORMS)
    for d in draws:
        d.emissive, d.metallic, d.roughness = np.ones(3, np.float32), 1.0, 1.0
    m = {"key": 10, "base_color": BASE, "normal": NORMAL, "emissive": LEVELS, "metallic_roughness": LEVELS}
    return Scene("levels", draws, [dict(m), dict(m)], sc.view, sc.proj)


def masked_scene(w, h):
    """The opaque icosphere, the masked torus in front of and through it (alpha from the base-colour ramp's A), and a masked grid of quads
    in front of both that spans more than the view (no base-colour bit: BaseColorAlpha x COLOR.a alone decides, COLOR.a rising with x)."""
    view, proj = R._camera(R.CAMERA_EYE, R.CAMERA_DIR, w, h)
    ico = textured_copy(R.icosphere_draw(translation=(0.1, 0.0, 3.3)), (0, 1), (1.0, 0.2, 0.1), -1.0, TRANSFORMS_A, cls=M.MaskDraw)
    torus = textured_copy(R.torus_draw(translation=(-0.2, 0.1, 3.0)), (0, 2), (0.2, 1.0, 0.3), 1.0, {"base_color": about_centre((1.5, 1.0))},
                          vertex_alpha=lambda p: 0.9 + 0.1 * np.sin(p[:, 1]), cls=M.MaskDraw, alpha=1.0625, cutoff=0.5)
    grid = quad_grid(np.linspace(-4.0, 4.0, 7), np.linspace(-3.0, 3.0, 7), lambda x, y: 1.5 + 0.04 * x - 0.03 * y, 11, base_color=np.array([0.8, 0.9, 0.3], np.float32),
                     emissive=np.array([1.0, 0.25, 0.0], np.float32), metallic=0.625, roughness=0.375, object_id=12)
    grid = textured_copy(grid, (0, 1), (1.0, 0.3, 0.1), 1.0, TRANSFORMS_B, vertex_alpha=lambda p: 0.6 + 0.13 * p[:, 0], cls=M.MaskDraw, alpha=0.9375, cutoff=0.625)
    mats = [_material(15), _material(M.ALPHA_MASK | 4 | 8, base_color=MASK_BASE), _material(M.ALPHA_MASK | 2 | 1)]
    return Scene("masked", [ico, torus, grid], mats, view, proj, masked=(1, 2), eye=R.CAMERA_EYE)


SCENES = {"textured": textured_scene, "textured strip": textured_strip_scene, "levels": levels_scene, "masked": masked_scene}
FORWARD_SCENES = ("textured", "masked")
_CASTS = {}


def cast_scene(name: str, w: int, h: int):
    """(scene, cast), cached per scene and target; the forward scenes' casts carry shade_forward's colour under scene_frame."""
    if (name, w, h) not in _CASTS:
        sc = SCENES[name](w, h)
        rc = cast(sc.draws, w, h, sc.view, sc.proj, sc.mats, sc.masked)
        if name in FORWARD_SCENES:
            shade_forward(rc, scene_frame(sc))
        _CASTS[(name, w, h)] = (sc, rc)
    return _CASTS[(name, w, h)]


def scene_frame(sc) -> FW.Frame:
    """A frame like forward_ref.soup_frame for a scene: the camera's eye, a light off every axis whose orthographic window holds the
    middle of the first two draws and not their rim, a 16 x 16 shadow map of three constant regions (so that the PCF compares flip along
    a few curves, not from texel to texel; the bilinear weights still blend across the regions' borders), shadow strength 0.75, an 8-texel 4-mip cube and the 128 x 32 LUT."""
    from unclerenderer_amd import hostmath, synth
    pts = np.concatenate([R._mesh(d)[0].reshape(-1, 3) @ R._m4(d.world)[:3, :3] + R._m4(d.world)[3, :3] for d in sc.draws[:2]])
    centre = 0.5 * (pts.min(axis=0) + pts.max(axis=0))
    radius = float(np.linalg.norm(pts - centre, axis=1).max())
    j, i = np.mgrid[0:16, 0:16]
    shadow = np.where(j >= 10, 0.5, np.where(i < 8, 1.0, 0.0)).astype(np.float32)  # lit, shadowed, and a band the surfaces' depths cross
    return FW.Frame(camera=np.asarray(sc.eye, np.float32), light_direction=np.array([0.3, 0.8, -0.45], np.float32), light_color=np.array([1.0, 0.95, 0.85], np.float32),
                    light_intensity=3.0, lvp=hostmath.light_view_projection(centre, 0.7 * radius, (-0.3, 0.8, -0.5)), shadow_strength=0.75, shadow_bias=0.002,
                    shadow=shadow, cube_bits=synth.env_cube_procedural(8, 4), env_base=8, env_mips=4, lut=synth.brdf_lut_procedural(128, 32))


def background(w: int, h: int) -> np.ndarray:
    """The HDR image in front of the forward pass: a finite pattern, different at every texel."""
    j, i = np.mgrid[0:h, 0:w]
    img = np.stack([0.25 + 0.001 * i, 0.5 + 0.002 * j, 0.125 + 0.0005 * (i + j), np.ones_like(i, np.float64)], axis=-1)
    return img.astype(np.float16).view(np.uint16)
