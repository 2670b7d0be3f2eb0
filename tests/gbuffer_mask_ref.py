"""The alpha-masked GBuffer rule restated in numpy: what ur_gbuffer_pass_masked must compute, to the byte.

The opaque selection is tests/gbuffer_ref.py's raster, called as it is; the vertex stage, the near clip with its weight rows, the piece
that covers a centre, the exact edge values, the quad partners' coordinates, the sampler and the resolve are tests/gbuffer_tex_ref.py's
(section 3.10). This file adds what section 3.11 adds: every fragment of the masked selection that passes the depth test (rule 2), its
alpha from COLOR.a, BaseColorAlpha and channel A of the base-colour map - the same sampler over a texture whose R, G, B are its A, read
as code / 255 - and the discard (rule 3), the per-texel maximum of (depth bits << 32) | key over the survivors (rule 4), the merge with
the opaque keys and the raised depth (rule 5), and the resolve over the final keys (rule 6), where a key names a slot through its own
selection. numpy float32 arithmetic is IEEE, one rounding per operation, no contraction.

The kernel evaluates alpha only for a fragment whose word is above the texel's current one; the maximum over the survivors does not
depend on that, so the restatement evaluates every passing fragment, a layer (the k-th largest word of every texel) at a time.

Accuracy over the seeded soups (tests/test_gbuffer_mask_ref.py prints them): with the alpha of every fragment evaluated a second time in
float64, the texels where float64 takes another probe count, level, tap or discard decision are left out (their share is capped at 2 %,
section 3.10's cap); on the others keys and depth are equal, and A and C stay within section 3.10's bounds.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from tests import depth_ref as D
from tests import gbuffer_ref as G
from tests import gbuffer_tex_ref as X
from tests import shadow_ref as S

ALPHA_MASK = 16  # UR_MATERIAL_ALPHA_MASK
F = np.float32


@dataclass
class MaskDraw(X.TexDraw):
    """A TexDraw with BaseColorAlpha, AlphaCutoff and AlphaMode (floats 106, 107 and dword 108 of ur_scene_constants)."""
    alpha: float = 1.0
    cutoff: float = 0.5
    alpha_mode: int = 1  # (not consulted by the rule: the material's bit is the pipeline)

    def constants(self) -> np.ndarray:
        c = super().constants()
        c[106], c[107] = self.alpha, self.cutoff
        c.view(np.uint32)[108] = self.alpha_mode
        return c


def alpha_texture(tex: X.Tex) -> X.Tex:
    """Channel A of a texture as the R, G, B of a UNORM one: gbuffer_tex_ref.sample on it is the sampler's alpha output, code / 255."""
    return X.Tex([np.repeat(level[:, :, 3:4], 4, axis=2) for level in tex.levels], False, tex.valid, tex.how)


def fragments(draws, view, proj, depth, w: int, h: int, flags: int, select, T: int):
    """Rule 2: every fragment of the selected draws that passes zs >= depth, as (texel, bits of zs, key) arrays, and stats[0:6] with
    gbuffer_ref's meanings. The loop is gbuffer_ref.gbuffer_pass' raster with the fragments kept instead of the largest key."""
    stats = np.zeros(6, np.int64)
    texel, zbits, keys = [], [], []
    depth = np.asarray(depth, F).reshape(h, w)
    for o, s in select:
        d = draws[s]
        if d.instance_count == 0:
            continue
        ntri = d.count() // 3
        raw = np.ascontiguousarray(d.vertices).reshape(-1).view(np.uint8)
        idx = np.ascontiguousarray(d.indices).reshape(-1).view(np.uint32)
        if d.index_format != S.R32_UINT or d.stride < G.VERTEX_BYTES or d.stride % 4 != 0 or ntri > (1 << T):
            stats[1] += ntri
            continue
        t = np.arange(ntri, dtype=np.int64)
        first = d.start_index + 3 * t
        in_ib = first + 2 < idx.size
        tri_idx = idx[np.minimum(first[:, None] + np.arange(3), max(idx.size - 1, 0))].astype(np.int64) if idx.size else np.zeros((ntri, 3), np.int64)
        vi = d.base_vertex + tri_idx
        in_vb = (vi >= 0) & (vi * d.stride + G.VERTEX_BYTES <= raw.size)
        flat = np.where(in_vb, vi, 0).reshape(-1)
        if raw.size >= 12:
            byte = flat[:, None] * d.stride + np.arange(12)
            pos = raw[np.minimum(byte, raw.size - 1)].reshape(-1, 12).copy().view(F).reshape(-1, 3)
        else:
            pos = np.zeros((flat.size, 3), F)
        W = np.asarray(d.world, F).reshape(4, 4)
        with np.errstate(all="ignore"):
            wv = [((pos[:, 0] * W[0, k] + pos[:, 1] * W[1, k]) + pos[:, 2] * W[2, k]) + W[3, k] for k in range(4)]
            clip = np.stack(D._mul(D._mul(wv, view), proj), axis=1).astype(F).reshape(ntri, 3, 4)
            supported = in_ib & in_vb.all(axis=1) & np.isfinite(clip).all(axis=(1, 2)) & (clip[:, :, 2] > 0).all(axis=1)
        stats[1] += int((~supported).sum())
        keep = np.flatnonzero(supported)
        poly, emit, n_out, _ = G.near_clip(clip[keep])
        stats[4] += int(((n_out == 1) | (n_out == 2)).sum())
        stats[5] += int((n_out == 3).sum())
        Xs, Ys, Zs = D.viewport(poly, w, h)
        with np.errstate(all="ignore"):
            bad = ~np.isfinite(Xs) | ~np.isfinite(Ys) | ~np.isfinite(Zs) | (np.abs(Xs) > D.GUARD_BAND) | (np.abs(Ys) > D.GUARD_BAND)
        for k in range(keep.size):
            key = ((o + 1) << T) | int(keep[k])
            for e in range(int(emit[k])):
                u = [0, 2 + e, 1 + e]
                if bad[k, u].any():
                    stats[2] += 1
                    continue
                f = G.raster(S.snap(Xs[k, u]), S.snap(Ys[k, u]), Zs[k, u], w, h)
                if f is None:
                    continue
                stats[0] += 1
                py, px, z = f[0], f[1], f[2]
                if not py.size:
                    continue
                with np.errstate(all="ignore"):
                    ok = z >= 0
                    zs = np.minimum(z, G.F1) + F(0.0)
                    if flags & G.QUANTIZE_D24:
                        zs = D.quantize_d24(zs)
                    ok &= zs >= depth[py, px]
                texel.append((py * w + px)[ok])
                zbits.append(zs[ok].astype(F).view(np.uint32))
                keys.append(np.full(int(ok.sum()), key, np.uint32))
    cat = lambda a, t: np.concatenate(a).astype(t) if a else np.zeros(0, t)  # noqa: E731
    return cat(texel, np.int64), cat(zbits, np.uint32), cat(keys, np.uint32), stats.astype(np.uint32)


def vertex_alpha(draws, g, keys_flat, T: int) -> np.ndarray:
    """COLOR.a (vertex byte 60) of the three vertices of every gathered texel's triangle: (n, 3)."""
    tri = (keys_flat[g["at"]] & np.uint32((1 << T) - 1)).astype(np.int64)
    out = np.zeros((g["at"].size, 3), F)
    for s in np.unique(g["slot"]):
        d = draws[int(s)]
        rows = np.flatnonzero(g["slot"] == s)
        raw = np.ascontiguousarray(d.vertices).reshape(-1).view(np.uint8)
        idx = np.ascontiguousarray(d.indices).reshape(-1).view(np.uint32)
        vi = d.base_vertex + idx[d.start_index + 3 * tri[rows][:, None] + np.arange(3)].astype(np.int64)
        byte = vi.reshape(-1)[:, None] * d.stride + 60 + np.arange(4)
        out[rows] = raw[byte].reshape(-1, 4).copy().view(F).reshape(-1, 3)
    return out


def alpha_test(draws, g, va, materials, ft=np.float32):
    """Rule 3 for the gathered fragments: (discarded (n,) bool, alpha (n,), sampled (n,) bool, N, L (n,), taps (n, 4, 2, 2)); N = 0 where
    the base-colour map is not sampled."""
    n = g["at"].size
    cs = g["cs"]
    odd_col, odd_row = (g["px"] & 1) == 1, (g["py"] & 1) == 1
    step_x, step_y = np.where(odd_col, -256, 256)[:, None], np.where(odd_row, -256, 256)[:, None]
    masked = np.zeros(n, bool)
    sampled = np.zeros(n, bool)
    N, L, taps = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros((n, 4, 2, 2), np.int64)
    with np.errstate(all="ignore"):
        b = X._weights(g["lam"], g["cw"], g["B"], ft)
        ca = (b[0] * va[:, 0].astype(ft) + b[1] * va[:, 1].astype(ft)) + b[2] * va[:, 2].astype(ft)
        alpha = cs[:, 106].astype(ft) * ca
        bx = X._weights(g["lam"] + step_x * g["dsx"], g["cw"], g["B"], ft)
        by = X._weights(g["lam"] + step_y * g["dsy"], g["cw"], g["B"], ft)
        uvc, uvx, uvy = X._mix(b, g["uv"], ft), X._mix(bx, g["uv"], ft), X._mix(by, g["uv"], ft)
    for s in np.unique(g["slot"]):
        m = materials[int(s)] if materials is not None and int(s) < len(materials) else None
        key = int(m.get("key", 0)) if m is not None else 0
        if not key & ALPHA_MASK:
            continue
        rows = np.flatnonzero(g["slot"] == s)
        masked[rows] = True
        tex = m.get("base_color") if key & X.BASE_COLOR else None
        if tex is None or not tex.valid:
            continue
        with np.errstate(all="ignore"):
            c = cs[rows]
            tu, tv = X.transform(c, 112, uvc[rows, 0], uvc[rows, 1], ft)
            xu, xv = X.transform(c, 112, uvx[rows, 0], uvx[rows, 1], ft)
            yu, yv = X.transform(c, 112, uvy[rows, 0], uvy[rows, 1], ft)
            oc, orow = odd_col[rows], odd_row[rows]
            dxu, dxv = np.where(oc, tu - xu, xu - tu), np.where(oc, tv - xv, xv - tv)
            dyu, dyv = np.where(orow, tu - yu, yu - tu), np.where(orow, tv - yv, yv - tv)
            sa, N[rows], L[rows], taps[rows] = X.sample(alpha_texture(tex), tu, tv, dxu, dxv, dyu, dyv, ft)
            alpha[rows] = alpha[rows] * sa[:, 0]
        sampled[rows] = True
    with np.errstate(all="ignore"):
        discarded = masked & (alpha < cs[:, 107].astype(ft))  # (false for a NaN on either side)
    return discarded, alpha, sampled, N, L, taps


def masked_pass(draws, view, proj, depth, w: int, h: int, materials=None, flags: int = 0, select=None, mask_select=(), key_triangle_bits: int = 0,
                command_count=None, precise: bool = False):
    """ur_gbuffer_pass_masked over the whole target (a band is rows of it). select / mask_select: gbuffer_ref.selection(...) of the opaque
    and the masked draws (select None: every slot). Returns gbuffer_ref.gbuffer_pass' dict without object_id, with `depth` (the raised
    depth), `keys64` (the winning masked word where it won, else 0), `won`, `mask_stats`, and `layers`: per layer the fragments' texels,
    discards and the sampler's choices. precise: the alpha of every fragment and the resolve a second time in float64 (`differs`: the
    texels where float64 took another choice in an alpha evaluation; `keys_f64`, `depth_f64`: the final keys and depth under float64's
    discard decisions; `shade64`)."""
    command_count = len(draws) if command_count is None else command_count
    T = G.key_bits(command_count, key_triangle_bits)
    depth = np.asarray(depth, F).reshape(h, w)
    mask_select = list(mask_select)
    opaque = G.gbuffer_pass(draws, view, proj, depth, w, h, flags=flags, select=select, key_triangle_bits=key_triangle_bits, command_count=command_count)
    ko = opaque["keys"].reshape(-1)
    texel, zbits, fkeys, mask_stats = fragments(draws, view, proj, depth, w, h, flags, mask_select, T)
    word = (zbits.astype(np.uint64) << np.uint64(32)) | fkeys.astype(np.uint64)
    # ---- rules 3-4: layer k holds the k-th largest word of every texel; the first survivor in that order is the maximum
    order = np.lexsort((np.iinfo(np.uint64).max - word, texel))
    texel, word = texel[order], word[order]
    start = np.r_[True, texel[1:] != texel[:-1]] if texel.size else np.zeros(0, bool)
    rank = np.arange(texel.size) - np.maximum.accumulate(np.where(start, np.arange(texel.size), 0)) if texel.size else np.zeros(0, np.int64)
    km, km64 = np.zeros(h * w, np.uint64), np.zeros(h * w, np.uint64)
    clipped_in_front = np.zeros(h * w, np.int64)
    differs = np.zeros(h * w, bool)
    layers = []
    slot_of = dict(mask_select)
    for k in range(int(rank.max()) + 1 if rank.size else 0):
        rows = np.flatnonzero(rank == k)
        img = np.zeros(h * w, np.uint32)
        img[texel[rows]] = (word[rows] & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        g = X.gather(draws, view, proj, img.reshape(h, w), w, h, slot_of, T)  # (g["at"] is ascending, and so is texel[rows])
        va = vertex_alpha(draws, g, img, T)
        discarded, alpha, sampled, N, L, taps = alpha_test(draws, g, va, materials)
        layer = {"texel": g["at"], "discarded": discarded, "sampled": sampled, "N": N, "alpha": alpha, "slot": g["slot"]}
        if precise:
            d64, _, _, N64, L64, taps64 = alpha_test(draws, g, va, materials, np.float64)
            take64 = ~d64 & (km64[g["at"]] == 0)
            km64[g["at"][take64]] = word[rows][take64]
            differs[g["at"]] |= (d64 != discarded) | (sampled & ((N64 != N) | (L64 != L) | (taps64 != taps).any(axis=(1, 2, 3))))
        take = ~discarded & (km[g["at"]] == 0)
        clipped_in_front[g["at"]] += discarded & (km[g["at"]] == 0)
        km[g["at"][take]] = word[rows][take]
        layers.append(layer)
    # ---- rule 5
    dbits = depth.reshape(-1).view(np.uint32)

    def merge(km):
        hi, lo = (km >> np.uint64(32)).astype(np.uint32), (km & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        wins = (km != 0) & ((hi > dbits) | (lo > ko))
        return wins, np.where(wins, lo, ko).astype(np.uint32), np.where(wins, hi, dbits).astype(np.uint32).view(F).reshape(h, w)

    wins, final, new_depth = merge(km)
    # ---- rule 6: the resolve of section 3.10 over the final keys; a masked key's ordinal is moved past every opaque one, so that one
    # table maps both selections' ordinals to their slots
    shift = 1 << (32 - T)
    virtual = final.astype(np.int64) + np.where(wins, np.int64(1) << 32, 0)
    slots = dict([(k, k) for k in range(len(draws))] if select is None else select)
    slots.update({o + shift: s for o, s in mask_select})
    g = X.gather(draws, view, proj, virtual.reshape(h, w), w, h, slots, T)
    mats = materials if materials is not None else []
    r = X.shade(g, view, mats)
    at = g["at"]
    clear_half = np.array([0, 0, 0, 0x3C00], np.uint16)
    out = {k: np.tile(clear_half, (h * w, 1)) for k in ("A", "B", "hdr")}
    out["C"] = np.full(h * w, 0xFF000000, np.uint32)
    for k in ("A", "B", "hdr"):
        out[k][at] = G._half(r[k])
    code = G.srgb_encode(r["albedo"])
    out["C"][at] = code[:, 0] | (code[:, 1] << 8) | (code[:, 2] << 16) | np.uint32(0xFF000000)
    out = {k: (v.reshape(h, w, 4) if v.ndim == 2 else v.reshape(h, w)) for k, v in out.items()}
    out.update({"keys": final.reshape(h, w), "depth": new_depth, "keys64": np.where(wins, km, np.uint64(0)).reshape(h, w), "won": int(wins.sum()),
                "wins": wins.reshape(h, w), "stats": opaque["stats"], "mask_stats": mask_stats, "layers": layers, "opaque_keys": opaque["keys"],
                "clipped_in_front": np.where(km != 0, clipped_in_front, 0).reshape(h, w), "gather": g, "shade32": r})
    if precise:
        out["shade64"] = X.shade(g, view, mats, np.float64)
        out["differs"] = differs.reshape(h, w)
        _, keys_f64, out["depth_f64"] = merge(km64)
        out["keys_f64"] = keys_f64.reshape(h, w)
    return out


# ---- inputs --------------------------------------------------------------------------------------------------------------------------

SOUPS = X.SOUPS


def masked_slots(count: int = X.SOUP_DRAWS):
    """The slots of the soups' masked selection: every third one."""
    return [k for k in range(count) if k % 3 == 2]


def soup(w: int, h: int, seed: int, triangles: int = 2000):
    """gbuffer_tex_ref.soup's commands as MaskDraws: COLOR.a seeded in [0.25, 1.25) per vertex, BaseColorAlpha in [0.8, 1.2) and AlphaCutoff
    in (0.2, 0.8) per command; AlphaMode is 1 on every second command whatever its material says."""
    rng = np.random.default_rng(seed + 4000)
    out = []
    for k, d in enumerate(X.soup(w, h, seed, triangles)):
        v = np.ascontiguousarray(d.vertices).view(F).reshape(-1, 16).copy()
        v[:, 15] = rng.uniform(0.25, 1.25, v.shape[0]).astype(F)
        out.append(MaskDraw(v.reshape(-1).view(np.uint8).copy(), d.indices, base_color=d.base_color, emissive=d.emissive, metallic=d.metallic, roughness=d.roughness,
                            object_id=d.object_id, transforms=d.transforms, alpha=float(F(rng.uniform(0.8, 1.2))), cutoff=float(F(rng.uniform(0.2, 0.8))),
                            alpha_mode=k & 1))
    return out


def soup_materials(seed: int, count: int = X.SOUP_DRAWS):
    """gbuffer_tex_ref.soup_materials (texture alpha is random bytes) with the masked slots on keys 16-31: slot k has key (k % 16) | 16, so
    the six of them cover a base-colour map, none, and one without bit 4 (slot 14 keeps key 14: nothing of it is discarded)."""
    mats = X.soup_materials(seed, count)
    for k in masked_slots(count):
        if k != 14:
            mats[k]["key"] |= ALPHA_MASK
    return mats


def soup_selections(count: int = X.SOUP_DRAWS):
    """(opaque, masked) as gbuffer_ref.selection lists over every slot's own ordinal."""
    masked = masked_slots(count)
    return [(k, k) for k in range(count) if k not in masked], [(k, k) for k in masked]
