"""The textured GBuffer rule restated in numpy: what ur_gbuffer_pass_materials must compute, to the byte.

The raster, the keys, the counters and the clear values are tests/gbuffer_ref.py's (section 3.9), called as they are. This file restates
the resolve per covered texel the way the kernel walks it - the winning triangle's three vertices, the near clip with its weight rows,
the piece that covers the centre, the exact edge values - and adds what section 3.10 adds: TEXCOORD and the vertex shader's tangent as
interpolated attributes, the quad partners' coordinates from the affine edge functions, ApplyTextureTransform per map, the footprint,
the 8.8 level of detail from the threshold table, up to four trilinear probes, and DeferredBasePass.hlsl's pixel shader for pipeline keys
0-15. numpy float32 arithmetic is IEEE, one rounding per operation, no contraction.

A texture is a Tex (levels of (h, w, 4) uint8, srgb); a material a dict {"key": k, "base_color" / "metallic_roughness" / "normal" /
"emissive": Tex or None}: a set bit whose Tex is None or `valid=False` counts as clear. gbuffer_pass(..., materials=[...]) takes one per
command slot; a slot past the list resolves as key 0.

With precise=True the resolve is evaluated a second time in float64 from the same fp32 vertex-stage values, integers and texel codes (the
two tables in double); the result carries, per covered texel and map, whether float64 took the same probe count, level and taps.

Accuracy over the seeded soups (tests/test_gbuffer_tex_ref.py prints them), on the texels where float64 takes the same N, L and taps
(the share left out is capped at 2 %): MEASURED_A_ULPS fp16 ulps of the float64 value in A, MEASURED_C_CODES codes in C.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from tests import depth_ref as D
from tests import gbuffer_ref as G
from tests import shadow_ref as S

NORMAL, METALLIC_ROUGHNESS, BASE_COLOR, EMISSIVE = 1, 2, 4, 8  # BuildPipelineKey's bits
MAPS = (("base_color", BASE_COLOR, 112), ("metallic_roughness", METALLIC_ROUGHNESS, 120), ("normal", NORMAL, 128), ("emissive", EMISSIVE, 136))
UNORM, UNORM_SRGB = 28, 29
F = np.float32
# (i + 0.5) / N - 0.5 as the kernel's fp32 literals
PROBE_OFFSETS = {1: [0.0], 2: [-0.25, 0.25], 3: [-0.33333334, 0.0, 0.33333334], 4: [-0.375, -0.125, 0.125, 0.375]}
COORD_LIMIT = 1073741824.0  # 2^30 texels: a coordinate beyond it, or not finite, counts as 0

MEASURED_A_ULPS = 29.74  # the 257 x 130 soup (1.35 on 64 x 64): a normal-mapped normal whose small component carries the sampler's fp32 weight error
MEASURED_C_CODES = 1
A_ULPS_BOUND = 128.0  # gbuffer_ref.bound: 4 x 29.74, rounded up to a power of two
C_CODES_BOUND = 4     # 4 x 1


@dataclass
class Tex:
    levels: list
    srgb: bool = False
    valid: bool = True
    how: str = "format"  # with valid=False, the way the device descriptor is broken: format, null, misaligned, width, height or mips

    @property
    def width(self):
        return self.levels[0].shape[1]

    @property
    def height(self):
        return self.levels[0].shape[0]


def random_texture(w: int, h: int, mips: int, srgb: bool, rng) -> Tex:
    """Every level filled with unrelated random bytes: a wrong level or a wrong blend cannot cancel out."""
    return Tex([rng.integers(0, 256, (max(1, h >> k), max(1, w >> k), 4), dtype=np.uint8) for k in range(mips)], srgb)


_TABLES = None


def tables():
    """(the sRGB decode table, the level-of-detail thresholds): the library's own bytes."""
    global _TABLES
    if _TABLES is None:
        from unclerenderer_amd import hostmath
        _TABLES = (hostmath.srgb_decode_table(), hostmath.lod_table())
    return _TABLES


def lod_reference() -> np.ndarray:
    return np.exp2(np.arange(1, 128, dtype=np.float64) / 128.0)


def level_of_detail(rho2, mips: int) -> np.ndarray:
    """The 8.8 fixed-point level of fp32 rho^2, clamped to [0, 256 (mips - 1)]: 128 e + (thresholds <= m) from the float's bits."""
    rho2 = np.asarray(rho2, F)
    bits = rho2.view(np.uint32).astype(np.int64)
    ef = (bits >> 23) & 255
    m = ((bits & 0x007FFFFF) | 0x3F800000).astype(np.uint32).view(F)
    count = (m[..., None] >= tables()[1]).sum(axis=-1)
    lmax = 256 * (mips - 1)
    L = np.clip(128 * (ef - 127) + count, 0, lmax)
    return np.where(ef == 255, lmax, np.where(ef == 0, 0, L)).astype(np.int64)


def level_of_detail64(rho2, mips: int) -> np.ndarray:
    """floor(256 log2 rho) in float64 with the same clamps and special cases."""
    rho2 = np.asarray(rho2, np.float64)
    lmax = 256 * (mips - 1)
    with np.errstate(all="ignore"):
        L = np.floor(128.0 * np.log2(rho2))
        L = np.where(np.isfinite(rho2), np.where(rho2 < 2.0 ** -126, 0, np.clip(L, 0, lmax)), lmax)
    return np.nan_to_num(L, nan=float(lmax)).astype(np.int64)


def transform(cs, at: int, u, v, ft):
    """ApplyTextureTransform with the constant vectors at floats [at, at + 8) of the block."""
    c = cs[:, at:at + 8].astype(ft)
    su, sv = u * c[:, 2], v * c[:, 3]
    ru, rv = su * c[:, 4] - sv * c[:, 5], su * c[:, 5] + sv * c[:, 4]
    return ru + c[:, 0], rv + c[:, 1]


def _wrap_pair(u, size: int, ft):
    with np.errstate(all="ignore"):
        x = u * ft(size) - ft(0.5)
        x = np.where(np.abs(x) <= COORD_LIMIT, x, ft(0.0)).astype(ft)
    x0 = np.floor(x)
    i0 = np.mod(x0.astype(np.int64), size)
    return i0, np.where(i0 + 1 == size, 0, i0 + 1), (x - x0).astype(ft), x0.astype(np.int64)


def _bilinear(tex: Tex, level: int, u, v, ft):
    """One bilinear sample of a level per row of (u, v): ((n, 3) R, G, B, (n, 2) the unwrapped first tap)."""
    img = tex.levels[level]
    hd, wd = img.shape[:2]
    x0, x1, fx, ux = _wrap_pair(u, wd, ft)
    y0, y1, fy, uy = _wrap_pair(v, hd, ft)
    if ft is np.float32:
        tab = tables()[0] if tex.srgb else (np.arange(256, dtype=F) / F(255.0)).astype(F)
    else:
        tab = G.srgb_decode(np.arange(256)) if tex.srgb else np.arange(256, dtype=np.float64) / 255.0
    t = lambda y, x: tab[img[y, x, :3]]  # noqa: E731
    a, b, d, e = t(y0, x0), t(y0, x1), t(y1, x0), t(y1, x1)
    top, bottom = a + fx[:, None] * (b - a), d + fx[:, None] * (e - d)
    return (top + fy[:, None] * (bottom - top)).astype(ft), np.stack([ux, uy], axis=1)


def sample(tex: Tex, u, v, dxu, dxv, dyu, dyv, ft=np.float32):
    """The static sampler of section 3.10 on n coordinates: (rgb (n, 3), N (n,), L (n,), taps (n, 4, 2, 2))."""
    n = u.shape[0]
    W, H, mips = tex.width, tex.height, len(tex.levels)
    with np.errstate(all="ignore"):
        axu, axv, ayu, ayv = dxu * ft(W), dxv * ft(H), dyu * ft(W), dyv * ft(H)
        px2, py2 = axu * axu + axv * axv, ayu * ayu + ayv * ayv
        ymajor = py2 > px2
        pmax2, pmin2 = np.where(ymajor, py2, px2), np.where(ymajor, px2, py2)
        N = np.where(pmax2 <= pmin2, 1, np.where(pmax2 <= ft(4.0) * pmin2, 2, np.where(pmax2 <= ft(9.0) * pmin2, 3, 4)))
        rho2 = (pmax2 / (N * N).astype(ft)).astype(ft)
    L = level_of_detail(rho2, mips) if ft is np.float32 else level_of_detail64(rho2, mips)
    d, f = L >> 8, ((L & 255).astype(ft) / ft(256.0)).astype(ft)
    mu, mv = np.where(ymajor, dyu, dxu), np.where(ymajor, dyv, dxv)
    out = np.zeros((n, 3), ft)
    taps = np.full((n, 4, 2, 2), -(2 ** 40), np.int64)
    for count in range(1, 5):
        for lv in range(mips):
            rows = np.flatnonzero((N == count) & (d == lv))
            if not rows.size:
                continue
            lv1 = min(lv + 1, mips - 1)
            total = None
            for i, o in enumerate(PROBE_OFFSETS[count]):
                with np.errstate(all="ignore"):
                    pu, pv = u[rows] + mu[rows] * ft(o), v[rows] + mv[rows] * ft(o)
                    s, t0 = _bilinear(tex, lv, pu, pv, ft)
                    hi, t1 = _bilinear(tex, lv1, pu, pv, ft)
                    s = (s + f[rows, None] * (hi - s)).astype(ft)  # (f == 0: s + 0 = s, the kernel skips the upper level)
                    total = s if total is None else (total + s).astype(ft)
                taps[rows, i, 0] = t0
                taps[rows, i, 1] = np.where((f[rows] != 0)[:, None], t1, -1)
            out[rows] = (total / ft(count)).astype(ft)
    return out, N, L, taps


# ---- the resolve ------------------------------------------------------------------------------------------------------------------------

def _sum3(a, b, c):
    return (a + b) + c


def _norm(v):
    return v / np.sqrt(_sum3(v[:, 0] * v[:, 0], v[:, 1] * v[:, 1], v[:, 2] * v[:, 2]))[:, None]


def _cover(X, Y, sx, sy):
    """Rules 3-4 of the reordered target-space triangles (n, 3) at the centres (sx, sy): (covered, snapped x, y, [E12, E20, E01])."""
    with np.errstate(all="ignore"):
        ok = (np.isfinite(X) & np.isfinite(Y) & (np.abs(X) <= D.GUARD_BAND) & (np.abs(Y) <= D.GUARD_BAND)).all(axis=1)
    xi, yi = S.snap(np.where(ok[:, None], X, 0)), S.snap(np.where(ok[:, None], Y, 0))
    x0, x1, x2 = xi.T
    y0, y1, y2 = yi.T
    A = (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0)
    E, inside = [], ok & (A > 0)
    for (ax, ay, bx, by) in ((x0, y0, x1, y1), (x1, y1, x2, y2), (x2, y2, x0, y0)):
        dx, dy = bx - ax, by - ay
        e = dx * (sy - ay) - dy * (sx - ax)
        inside &= np.where((dy < 0) | ((dy == 0) & (dx > 0)), e >= 0, e > 0)
        E.append(e)
    return inside, xi, yi, np.stack([E[1], E[2], E[0]], axis=1)


def gather(draws, view, proj, keys, w: int, h: int, slot_of: dict, T: int):
    """Per covered texel, what the kernel loads and derives in the vertex stage and the raster (all fp32 / integer): a dict."""
    flat = keys.reshape(-1)
    at = np.flatnonzero(flat)
    n = at.size
    ordinal, tri = (flat[at] >> np.uint32(T)).astype(np.int64) - 1, (flat[at] & np.uint32((1 << T) - 1)).astype(np.int64)
    slot = np.array([slot_of[int(o)] for o in ordinal], np.int64)
    vert, Wm, cs = np.zeros((n, 3, 16), F), np.zeros((n, 16), F), np.zeros((n, G.CONSTANT_FLOATS), F)
    for s in np.unique(slot):
        d = draws[int(s)]
        rows = np.flatnonzero(slot == s)
        raw = np.ascontiguousarray(d.vertices).reshape(-1).view(np.uint8)
        idx = np.ascontiguousarray(d.indices).reshape(-1).view(np.uint32)
        vi = d.base_vertex + idx[d.start_index + 3 * tri[rows][:, None] + np.arange(3)].astype(np.int64)
        byte = vi.reshape(-1)[:, None] * d.stride + np.arange(G.VERTEX_BYTES)
        vert[rows] = raw[byte].reshape(-1, G.VERTEX_BYTES).copy().view(F).reshape(-1, 3, 16)
        Wm[rows], cs[rows] = np.asarray(d.world, F).reshape(-1), d.constants()
    W4 = Wm.reshape(n, 4, 4)
    with np.errstate(all="ignore"):
        pos, nrm, tan = vert[:, :, 0:3], vert[:, :, 3:6], vert[:, :, 8:12]
        wv = [((pos[:, :, 0] * W4[:, None, 0, k] + pos[:, :, 1] * W4[:, None, 1, k]) + pos[:, :, 2] * W4[:, None, 2, k]) + W4[:, None, 3, k] for k in range(4)]
        clip = np.stack(D._mul(D._mul([a.reshape(-1) for a in wv], view), proj), axis=1).astype(F).reshape(n, 3, 4)
        rot = lambda a: np.stack([(a[:, :, 0] * W4[:, None, 0, k] + a[:, :, 1] * W4[:, None, 1, k]) + a[:, :, 2] * W4[:, None, 2, k] for k in range(3)], axis=2).astype(F)  # noqa: E731
        wn, wt = rot(nrm), rot(tan)
        wt = (wt / np.sqrt(_sum3(wt[:, :, 0] * wt[:, :, 0], wt[:, :, 1] * wt[:, :, 1], wt[:, :, 2] * wt[:, :, 2]))[:, :, None]).astype(F)
        wp = np.stack(wv[:3], axis=2).astype(F)
    poly, emit, n_out, B = G.near_clip(clip)
    X, Y, _ = D.viewport(poly, w, h)
    px, py = at % w, at // w
    sx, sy = 256 * px + 128, 256 * py + 128
    first, second = [0, 2, 1], [0, 3, 2]
    in0, xi0, yi0, lam0 = _cover(X[:, first], Y[:, first], sx, sy)
    _, xi1, yi1, lam1 = _cover(X[:, second], Y[:, second], sx, sy)
    sec = ~in0 & (n_out == 1)
    pick = lambda a, b: np.where(sec.reshape((-1,) + (1,) * (a.ndim - 1)), b, a)  # noqa: E731
    xi, yi, lam = pick(xi0, xi1), pick(yi0, yi1), pick(lam0, lam1)
    x0, x1, x2 = xi.T
    y0, y1, y2 = yi.T
    return {"at": at, "slot": slot, "px": px, "py": py, "lam": lam, "second": sec,
            "dsx": np.stack([-(y2 - y1), -(y0 - y2), -(y1 - y0)], axis=1), "dsy": np.stack([x2 - x1, x0 - x2, x1 - x0], axis=1),
            "cw": pick(poly[:, first, 3], poly[:, second, 3]), "B": pick(B[:, first], B[:, second]),
            "wn": wn, "wp": wp, "col": vert[:, :, 12:15], "uv": vert[:, :, 6:8], "tan": np.concatenate([wt, tan[:, :, 3:4]], axis=2), "cs": cs}


def _weights(lam, cw, B, ft):
    with np.errstate(all="ignore"):
        q = lam.astype(ft) / cw.astype(ft)
        g = q / _sum3(q[:, 0], q[:, 1], q[:, 2])[:, None]
        Bf = B.astype(ft)
        return [_sum3(g[:, 0] * Bf[:, 0, j], g[:, 1] * Bf[:, 1, j], g[:, 2] * Bf[:, 2, j]) for j in range(3)]


def _mix(b, a, ft):
    return np.stack([_sum3(b[0] * a[:, 0, k].astype(ft), b[1] * a[:, 1, k].astype(ft), b[2] * a[:, 2, k].astype(ft)) for k in range(a.shape[2])], axis=1)


def shade(g, view, materials, ft=np.float32):
    """The resolve of the gathered texels in `ft` arithmetic: dict of A (n, 4), B (n, 4), albedo (n, 3), hdr (n, 4) unrounded, and per map
    name the rows it was sampled on with their N, L and taps, and `bits`, the effective key per texel."""
    n = g["at"].size
    V = np.asarray(view, F).reshape(4, 4).astype(ft)
    cs = g["cs"]
    odd_col, odd_row = (g["px"] & 1) == 1, (g["py"] & 1) == 1
    step_x, step_y = np.where(odd_col, -256, 256)[:, None], np.where(odd_row, -256, 256)[:, None]
    with np.errstate(all="ignore"):
        b = _weights(g["lam"], g["cw"], g["B"], ft)
        bx = _weights(g["lam"] + step_x * g["dsx"], g["cw"], g["B"], ft)
        by = _weights(g["lam"] + step_y * g["dsy"], g["cw"], g["B"], ft)
        nrm, wpos, colour, tan = _mix(b, g["wn"], ft), _mix(b, g["wp"], ft), _mix(b, g["col"], ft), _mix(b, g["tan"], ft)
        uvc, uvx, uvy = _mix(b, g["uv"], ft), _mix(bx, g["uv"], ft), _mix(by, g["uv"], ft)
    bits = np.zeros(n, np.int64)
    samples, info = {}, {}
    for name, bit, at in MAPS:
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
                tu, tv = transform(c, at, uvc[rows, 0], uvc[rows, 1], ft)
                xu, xv = transform(c, at, uvx[rows, 0], uvx[rows, 1], ft)
                yu, yv = transform(c, at, uvy[rows, 0], uvy[rows, 1], ft)
                oc, orow = odd_col[rows], odd_row[rows]
                dxu, dxv = np.where(oc, tu - xu, xu - tu), np.where(oc, tv - xv, xv - tv)
                dyu, dyv = np.where(orow, tu - yu, yu - tu), np.where(orow, tv - yv, yv - tv)
            rgb, N, L, taps = sample(tex, tu, tv, dxu, dxv, dyu, dyv, ft)
            samples[name][rows] = rgb
            info.setdefault(name, []).append((rows, N, L, taps, np.stack([tu, tv, xu, xv, yu, yv], axis=1)))
    with np.errstate(all="ignore"):
        vn = _norm(nrm)
        wnrm = vn.copy()
        use = (bits & NORMAL) != 0
        if use.any():
            T3, tw = tan[:, :3], tan[:, 3]
            dt = _sum3(vn[:, 0] * T3[:, 0], vn[:, 1] * T3[:, 1], vn[:, 2] * T3[:, 2])
            t = _norm(T3 - vn * dt[:, None])
            c = np.stack([vn[:, 1] * t[:, 2] - vn[:, 2] * t[:, 1], vn[:, 2] * t[:, 0] - vn[:, 0] * t[:, 2], vn[:, 0] * t[:, 1] - vn[:, 1] * t[:, 0]], axis=1)
            bt = _norm(c) * tw[:, None]
            nm = samples["normal"]
            nr, ng = nm[:, 0] * ft(2.0) - ft(1.0), nm[:, 1] * ft(2.0) - ft(1.0)
            one_minus = ft(1.0) - (nr * nr + ng * ng)
            nz = np.sqrt(np.where(one_minus > 0, np.minimum(one_minus, ft(1.0)), ft(0.0)))
            flat = np.sqrt((nr * nr + ng * ng) + nz * nz) < ft(1e-5)
            e0, e1, e2 = np.where(flat, ft(0.0), nr), np.where(flat, ft(0.0), ng), np.where(flat, ft(1.0), nz)
            wn = np.stack([_sum3(e0 * t[:, k], e1 * bt[:, k], e2 * vn[:, k]) for k in range(3)], axis=1)
            wnrm = np.where(use[:, None], _norm(wn), vn)
        m = np.stack([_sum3(wnrm[:, 0] * V[0, k], wnrm[:, 1] * V[1, k], wnrm[:, 2] * V[2, k]) for k in range(3)], axis=1)
        normal = _norm(m)
        view_depth = -(_sum3(wpos[:, 0] * V[0, 2], wpos[:, 1] * V[1, 2], wpos[:, 2] * V[2, 2]) + V[3, 2])
        albedo = cs[:, 64:67].astype(ft) * colour
        albedo = np.where(((bits & BASE_COLOR) != 0)[:, None], albedo * samples["base_color"], albedo)
        mr = samples["metallic_roughness"]
        has_mr = (bits & METALLIC_ROUGHNESS) != 0
        metallic = np.where(has_mr, cs[:, 104].astype(ft) * mr[:, 2], cs[:, 104].astype(ft))
        roughness = np.where(has_mr, cs[:, 105].astype(ft) * mr[:, 1], cs[:, 105].astype(ft))
        emissive = np.where(((bits & EMISSIVE) != 0)[:, None], cs[:, 80:83].astype(ft) * samples["emissive"], cs[:, 80:83].astype(ft))
    one = np.ones(n, ft)
    return {"A": np.concatenate([normal, view_depth[:, None]], axis=1), "B": np.stack([np.full(n, ft(F(0.04))), metallic, roughness, one], axis=1),
            "albedo": albedo, "hdr": np.concatenate([emissive, one[:, None]], axis=1), "bits": bits, "info": info}


def gbuffer_pass(draws, view, proj, depth, w: int, h: int, materials=None, flags: int = 0, select=None, key_triangle_bits: int = 0,
                 command_count=None, precise: bool = False):
    """ur_gbuffer_pass_materials over the whole target (a band is rows of it): gbuffer_ref.gbuffer_pass' dict. materials None: that call."""
    base = G.gbuffer_pass(draws, view, proj, depth, w, h, flags=flags, select=select, key_triangle_bits=key_triangle_bits, command_count=command_count)
    if materials is None:
        return base
    command_count = len(draws) if command_count is None else command_count
    T = G.key_bits(command_count, key_triangle_bits)
    slot_of = dict([(k, k) for k in range(len(draws))] if select is None else select)
    g = gather(draws, view, proj, base["keys"], w, h, slot_of, T)
    r = shade(g, view, materials)
    out = {k: v.copy() for k, v in base.items()}
    at = g["at"]
    for k, name in (("A", "A"), ("B", "B"), ("hdr", "hdr")):
        out[k].reshape(-1, 4)[at] = G._half(r[name])
    code = G.srgb_encode(r["albedo"])
    out["C"].reshape(-1)[at] = code[:, 0] | (code[:, 1] << 8) | (code[:, 2] << 16) | np.uint32(0xFF000000)
    out["gather"], out["shade32"] = g, r
    if precise:
        out["shade64"] = shade(g, view, materials, np.float64)
    return out


def same_choices(out):
    """Per covered texel: float64 took the same N, L and taps as fp32 on every map it sampled."""
    ok = np.ones(out["gather"]["at"].size, bool)
    for name, runs in out["shade32"]["info"].items():
        for (rows, N, L, taps, _), (rows64, N64, L64, taps64, _) in zip(runs, out["shade64"]["info"][name]):
            ok[rows] &= (N == N64) & (L == L64) & (taps == taps64).all(axis=(1, 2, 3))
    return ok


def accuracy(out):
    """(the share of textured texels left out, the largest error of a channel of A in fp16 ulps of the float64 value, the largest
    difference of a code of C) over the texels where float64 takes the same N, L and taps."""
    ok = same_choices(out)
    textured = out["shade32"]["bits"] != 0
    a64 = out["shade64"]["A"]
    with np.errstate(all="ignore"):
        a16 = out["shade32"]["A"].astype(F).astype(np.float16).astype(np.float64)
        ulp = np.exp2(np.floor(np.log2(np.maximum(np.abs(a64), 2.0 ** -14))) - 10)
        err = np.abs(a16 - a64) / ulp
        fin = np.isfinite(a64) & np.isfinite(a16) & ok[:, None]
        c32 = G.srgb_encode(out["shade32"]["albedo"])
        c64 = G.srgb_encode(out["shade64"]["albedo"], G.table().astype(np.float64))
        good = np.isfinite(out["shade64"]["albedo"]) & ok[:, None]
    diff = np.abs(c32.astype(np.int64) - c64.astype(np.int64))[good]
    left_out = float((~ok & textured).sum()) / max(int(textured.sum()), 1)
    return left_out, float(err[fin].max()) if fin.any() else 0.0, int(diff.max()) if diff.size else 0


# ---- inputs --------------------------------------------------------------------------------------------------------------------------

TEXTURE_SHAPES = [(16, 16, 5), (13, 7, 4), (1, 1, 1), (8, 4, 1)]
# (w, h, mips) at the ends of ur_texture2d's ranges: the largest dimension each way, a chain one level longer than its last shrinking
# level, sizes that are no power of two, and the largest texture the tests upload (8 MB at level 0)
EDGE_SHAPES = [(65535, 1, 1), (1, 65535, 16), (65535, 2, 17), (1000, 600, 10), (2048, 1024, 12), (3, 4099, 13)]
SOUPS = [(64, 64, 1), (257, 130, 2)]
SOUP_DRAWS = 18
UV_SEED = 2000  # (chosen so that float64 takes other taps than fp32 on at most 2 % of the textured texels of both soups)


def soup(w: int, h: int, seed: int, triangles: int = 2000):
    """gbuffer_ref.soup's supported geometry re-cut into SOUP_DRAWS commands (so that every pipeline key has a command) with seeded
    TEXCOORDs - a scale per triangle, log-uniform from 1/4 to 64 texture repeats across it, which with the soup's triangle sizes reaches
    both level clamps and probe counts 2-4; 8 % of the triangles carry TEXCOORD (0, 0) at all three vertices, which gives N = 1 (an exactly
    isotropic footprint otherwise needs exact arithmetic: the hand cases have it) -, seeded tangents, and per-command texture transforms (one rotated, one scaled up)."""
    rng = np.random.default_rng(seed + UV_SEED)
    pos, rest = [], []
    for d in G.soup(w, h, seed, triangles):
        if d.stride != G.VERTEX_BYTES:
            continue
        v = np.ascontiguousarray(d.vertices).view(F).reshape(-1, 16)
        idx = np.ascontiguousarray(d.indices).view(np.uint32)[d.start_index:d.start_index + (d.count() // 3) * 3].astype(np.int64) + d.base_vertex
        tri = v[idx].copy()
        tri[:, 0:3] += np.asarray(d.world, F).reshape(4, 4)[3, :3]
        pos.append(tri)
    tri = np.concatenate(pos).reshape(-1, 3, 16)
    nt = tri.shape[0]
    scale = np.exp(rng.uniform(np.log(1.0 / 4.0), np.log(64.0), nt))
    tri[:, :, 6:8] = (rng.uniform(-2.0, 2.0, (nt, 1, 2)) + rng.uniform(-0.5, 0.5, (nt, 3, 2)) * scale[:, None, None]).astype(F)
    tri[rng.random(nt) < 0.08, :, 6:8] = 0.0  # TEXCOORD (0, 0) at all three vertices: exactly no footprint, the one robust way to N = 1
    tri[:, :, 8:11] = rng.normal(size=(nt, 3, 3)).astype(F)
    tri[:, :, 11] = rng.choice([-1.0, 1.0], (nt, 1)).astype(F)
    cuts = np.linspace(0, nt, SOUP_DRAWS + 1).astype(int)
    out = []
    for k in range(SOUP_DRAWS):
        t = tri[cuts[k]:cuts[k + 1]].reshape(-1, 16)
        g = TexDraw(t.reshape(-1).view(np.uint8).copy(), np.arange(t.shape[0], dtype=np.uint32),
                    base_color=rng.uniform(0.05, 1.0, 3).astype(F), emissive=rng.uniform(0.0, 4.0, 3).astype(F),
                    metallic=float(F(rng.uniform())), roughness=float(F(rng.uniform(0.05, 1.0))), object_id=int(rng.integers(1, 2 ** 32)))
        if k % 3 == 1:
            a = rng.uniform(0, 2 * np.pi)
            g.transforms = {name: (rng.uniform(-1, 1, 2), rng.uniform(0.5, 2.0, 2), (np.cos(a), np.sin(a))) for name, _, _ in MAPS}
        out.append(g)
    return out


@dataclass
class TexDraw(G.GDraw):
    """A GDraw with the four texture transforms: name -> (offset (2), scale (2), rotation (cos, sin)); default identity."""
    transforms: dict = None

    def constants(self) -> np.ndarray:
        c = super().constants()
        for name, _, at in MAPS:
            off, sc, rot = (self.transforms or {}).get(name, ((0, 0), (1, 1), (1, 0)))
            c[at:at + 4] = [off[0], off[1], sc[0], sc[1]]
            c[at + 4:at + 8] = [rot[0], rot[1], 0, 0]
        return c


def soup_materials(seed: int, count: int = SOUP_DRAWS, shapes=None):
    """A material per command cycling through keys 0-15 (command k: key k % 16), its four textures cycling through `shapes`
    (TEXTURE_SHAPES unless given), sRGB for base colour and emissive."""
    shapes = TEXTURE_SHAPES if shapes is None else shapes
    rng = np.random.default_rng(seed + 3000)
    out = []
    for k in range(count):
        m = {"key": k % 16}
        for j, (name, _, _) in enumerate(MAPS):
            tw, th, mips = shapes[(k + j) % len(shapes)]
            m[name] = random_texture(tw, th, mips, name in ("base_color", "emissive"), rng)
        out.append(m)
    return out
