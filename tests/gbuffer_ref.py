"""The GBuffer rule restated in numpy: what ur_gbuffer_pass must compute, to the byte.

The draws, their selections, the vertex rule, the near clip, the viewport, facing, coverage and the depth plane are tests/depth_ref.py's
(section 3.8) and tests/shadow_ref.py's (section 3.7); this file adds the 64-byte vertex, the key, the GREATER_EQUAL test against a given
depth, the per-texel maximum key, and the resolve: weight rows through the near clip, perspective-correct barycentrics from the exact
integer edge values, the interpolated attributes, the pixel shader of pipeline key 0 and the target encodings. numpy float32 arithmetic
is IEEE, one rounding per operation, no contraction, division and square root included.

gbuffer_pass(...) returns a dict: keys, A, B, hdr (uint16 views of fp16), C, object_id (uint32) and stats[0:6]; stats[3] is structural
and stays 0 here. With precise=True the barycentrics, the attributes and the pixel shader are evaluated in float64 from the same fp32
vertices, weight rows and integers, and A / albedo come back unrounded ("A64", "albedo64") beside the fp32 result.

Accuracy over the seeded soups (SOUPS below, tests/test_gbuffer_ref.py prints them): the largest error of a channel of A against the
float64 value = MEASURED_A_ULPS fp16 ulps of that value (the fp16 rounding of the fp32 result included), the largest difference of a
code of C = MEASURED_C_CODES. The bounds are 4 x that, rounded up to a power of two, and never below 1.
"""
from __future__ import annotations

from dataclasses import dataclass, field, replace

import numpy as np

from tests import depth_ref as D
from tests import shadow_ref as S

VERTEX_BYTES = 64
CONSTANT_FLOATS = 152  # ur_scene_constants, 608 bytes
QUANTIZE_D24 = D.QUANTIZE_D24
MEASURED_A_ULPS = 0.5154  # the 257 x 130 soup (0.5017 on 64 x 64): the fp16 rounding's half ulp and 0.015 ulp of fp32 error
MEASURED_C_CODES = 0
A_ULPS_BOUND = 4.0        # 4 x 0.5154 = 2.06, rounded up to a power of two
C_CODES_BOUND = 1         # 4 x 0 = 0: never below 1 code
F1 = np.float32(1.0)


@dataclass
class GDraw(S.Draw):
    """A Draw whose vertices are the reference's 64 bytes and whose constant block is a whole ur_scene_constants."""
    base_color: np.ndarray = field(default_factory=lambda: np.ones(3, np.float32))
    emissive: np.ndarray = field(default_factory=lambda: np.zeros(3, np.float32))
    metallic: float = 0.0
    roughness: float = 1.0
    object_id: int = 0

    def constants(self) -> np.ndarray:
        c = np.zeros(CONSTANT_FLOATS, np.float32)
        c[0:16] = np.asarray(self.world, np.float32).reshape(-1)
        c[64:67] = self.base_color
        c[80:83] = self.emissive
        c[104], c[105] = self.metallic, self.roughness
        c.view(np.uint32)[148] = self.object_id
        return c


def vertex_buffer(positions, normals=None, colors=None, fill: float = 7.0) -> np.ndarray:
    """64-byte vertices: POSITION at byte 0, NORMAL at 12, TEXCOORD at 24, TANGENT at 32, COLOR at 48; raw bytes."""
    p = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
    v = np.full((p.shape[0], 16), np.float32(fill), np.float32)
    v[:, 0:3] = p
    v[:, 3:6] = [0, 0, -1] if normals is None else np.asarray(normals, np.float32).reshape(-1, 3)
    v[:, 12:16] = 1.0
    if colors is not None:
        v[:, 12:15] = np.asarray(colors, np.float32).reshape(-1, 3)
    return v.reshape(-1).view(np.uint8).copy()


def as_device_draw(d: GDraw) -> S.Draw:
    """The Draw tests/shadow_gpu.py uploads: its constant buffer is the whole block."""
    return S.Draw(d.vertices, d.indices, d.constants(), d.stride, d.index_count, d.instance_count, d.start_index, d.base_vertex, d.index_format)


def key_bits(command_count: int, key_triangle_bits: int = 0) -> int:
    """T: the key's triangle bits."""
    return key_triangle_bits if key_triangle_bits else 32 - int(command_count).bit_length()


def selection(command_count: int, visible=None, index_base: int = 0, ranges=None):
    """[(ordinal, slot)] of a ur_raster_draws selection: the ordinal is the slot, or the position in the visible list."""
    if visible is not None:
        idx, cnt = visible
        out = []
        for k in range(min(int(cnt), command_count)):
            s = int((np.uint32(np.asarray(idx, np.uint32)[k]) - np.uint32(index_base)).astype(np.uint32))
            if s < command_count:
                out.append((k, s))
        return out
    return [(s, s) for s in S.selected_slots(command_count, ranges=ranges)]


def srgb_encode_reference() -> np.ndarray:
    """The 255 thresholds in float64: entry c - 1 is the linear value of sRGB (c - 0.5) / 255."""
    v = (np.arange(1, 256, dtype=np.float64) - 0.5) / 255.0
    return np.where(v <= 0.04045, v / 12.92, ((v + 0.055) / 1.055) ** 2.4)


def srgb_decode(codes) -> np.ndarray:
    v = np.asarray(codes, np.float64) / 255.0
    return np.where(v <= 0.04045, v / 12.92, ((v + 0.055) / 1.055) ** 2.4)


_TABLE = None


def table() -> np.ndarray:
    """The library's own bytes (ur_host_srgb_encode_table)."""
    global _TABLE
    if _TABLE is None:
        from unclerenderer_amd import hostmath
        _TABLE = hostmath.srgb_encode_table()
    return _TABLE


def srgb_encode(x, tab=None) -> np.ndarray:
    """The number of entries with x >= entry; a NaN gives 0."""
    tab = table() if tab is None else tab
    with np.errstate(invalid="ignore"):
        return (np.asarray(x)[..., None] >= tab).sum(axis=-1).astype(np.uint32)


def near_clip(c: np.ndarray):
    """depth_ref.near_clip with the weight rows: (poly (n, 4, 4), emit, n_out, B (n, 4, 3)) - B[:, v, j] is the weight of original vertex
    j in polygon vertex v: a unit row for an original vertex, 1 - t at i and t at o for a new vertex on i -> o."""
    poly, emit, n_out = D.near_clip(c)
    n = c.shape[0]
    with np.errstate(all="ignore"):
        d = (c[:, :, 3] - c[:, :, 2]).astype(np.float32)
        out = d < 0
        rot = np.where(n_out == 1, np.where(out[:, 0], 1, np.where(out[:, 1], 2, 0)),
                       np.where(n_out == 2, np.where(~out[:, 0], 0, np.where(~out[:, 1], 1, 2)), 0))
        rows = np.arange(n)
        ia, ib, ic = rot % 3, (rot + 1) % 3, (rot + 2) % 3
        da, db, dc = d[rows, ia], d[rows, ib], d[rows, ic]
        one, two, whole = n_out == 1, n_out == 2, n_out == 0
        unit = np.eye(3, dtype=np.float32)

        def new(i, o, di, do):
            t = (di / (di - do)).astype(np.float32)
            r = np.zeros((n, 3), np.float32)
            r[rows, i] = F1 - t
            r[rows, o] = t
            return r

        p = new(np.where(one, ib, ia), np.where(one, ic, ib), np.where(one, db, da), np.where(one, dc, db))
        q = new(ia, ic, da, dc)
        B = np.stack([unit[ia], np.where(two[:, None], p, unit[ib]), np.where(whole[:, None], unit[ic], np.where(one[:, None], p, q)), q], axis=1)
    return poly, emit, n_out, B.astype(np.float32)


def raster(xi, yi, z, w: int, h: int):
    """Rules 3-5 of section 3.7 for one reordered triangle: None when A <= 0, else (py, px, z fp32 before the clamp, E01, E12, E20)."""
    x0, x1, x2 = (int(v) for v in xi)
    y0, y1, y2 = (int(v) for v in yi)
    A = (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0)
    if A <= 0:
        return None
    px0, px1 = max(-((128 - min(x0, x1, x2)) // 256), 0), min((max(x0, x1, x2) - 128) // 256, w - 1)
    py0, py1 = max(-((128 - min(y0, y1, y2)) // 256), 0), min((max(y0, y1, y2) - 128) // 256, h - 1)
    if px0 > px1 or py0 > py1:
        e = np.zeros(0, np.int64)
        return e, e, np.zeros(0, np.float32), e, e, e
    sx = 256 * np.arange(px0, px1 + 1, dtype=np.int64) + 128
    sy = 256 * np.arange(py0, py1 + 1, dtype=np.int64) + 128
    inside, E = None, []
    for (ax, ay, bx, by) in ((x0, y0, x1, y1), (x1, y1, x2, y2), (x2, y2, x0, y0)):
        dx, dy = bx - ax, by - ay
        e = (dx * (sy - ay))[:, None] - (dy * (sx - ax))[None, :]
        ok = (e >= 0) if (dy < 0 or (dy == 0 and dx > 0)) else (e > 0)
        inside = ok if inside is None else inside & ok
        E.append(e)
    iy, ix = np.nonzero(inside)
    e01, e12, e20 = (E[k][iy, ix] for k in range(3))
    z0, z1, z2 = (np.float32(v) for v in z)
    with np.errstate(all="ignore"):
        inv = F1 / np.float32(A)
        k1, k2 = (z1 - z0) * inv, (z2 - z0) * inv
        zz = (z0 + (e20.astype(np.float32) * k1 + e01.astype(np.float32) * k2)).astype(np.float32)
    return iy + py0, ix + px0, zz, e01, e12, e20


def _sum3(a, b, c):
    return (a + b) + c


def shade(lam, cw, B, wn, wp, col, consts, view, ft=np.float32):
    """The resolve of n texels from their edge values lam (n, 3) int64, clip w cw (n, 3), weight rows B (n, 3 [k], 3 [j]) of the reordered
    triangle, per-vertex world normals, world positions and colours (n, 3 [j], 3) and constant blocks (n, 152): (A (n, 4), albedo (n, 3)) in
    `ft` arithmetic."""
    V = np.asarray(view, np.float32).reshape(4, 4).astype(ft)
    with np.errstate(all="ignore"):
        q = lam.astype(ft) / cw.astype(ft)
        s = _sum3(q[:, 0], q[:, 1], q[:, 2])
        g = q / s[:, None]
        Bf = B.astype(ft)
        b = [_sum3(g[:, 0] * Bf[:, 0, j], g[:, 1] * Bf[:, 1, j], g[:, 2] * Bf[:, 2, j]) for j in range(3)]
        mix = lambda a: np.stack([_sum3(b[0] * a[:, 0, k].astype(ft), b[1] * a[:, 1, k].astype(ft), b[2] * a[:, 2, k].astype(ft)) for k in range(3)], axis=1)  # noqa: E731
        n, wpos, colour = mix(wn), mix(wp), mix(col)
        vn = n / np.sqrt(_sum3(n[:, 0] * n[:, 0], n[:, 1] * n[:, 1], n[:, 2] * n[:, 2]))[:, None]
        m = np.stack([_sum3(vn[:, 0] * V[0, k], vn[:, 1] * V[1, k], vn[:, 2] * V[2, k]) for k in range(3)], axis=1)
        normal = m / np.sqrt(_sum3(m[:, 0] * m[:, 0], m[:, 1] * m[:, 1], m[:, 2] * m[:, 2]))[:, None]
        view_depth = -(_sum3(wpos[:, 0] * V[0, 2], wpos[:, 1] * V[1, 2], wpos[:, 2] * V[2, 2]) + V[3, 2])
        albedo = consts[:, 64:67].astype(ft) * colour
    return np.concatenate([normal, view_depth[:, None]], axis=1), albedo


def _half(x) -> np.ndarray:
    with np.errstate(all="ignore"):
        return np.asarray(x, np.float32).astype(np.float16).view(np.uint16)


def gbuffer_pass(draws, view, proj, depth, w: int, h: int, flags: int = 0, select=None, key_triangle_bits: int = 0, command_count=None,
                 precise: bool = False):
    """ur_gbuffer_pass over the whole target (a band is rows of it): see the module docstring. select: selection(...), default every slot."""
    command_count = len(draws) if command_count is None else command_count
    T = key_bits(command_count, key_triangle_bits)
    keys = np.zeros((h, w), np.uint32)
    stats = np.zeros(6, np.int64)
    tris = {}   # key -> the triangle's per-vertex data
    frags = {}  # (key, piece) -> (flat texel indices, E01, E12, E20) of a drawn piece
    depth = np.asarray(depth, np.float32).reshape(h, w)
    for o, s in ([(k, k) for k in range(len(draws))] if select is None else select):
        d = draws[s]
        if d.instance_count == 0:
            continue
        ntri = d.count() // 3
        raw = np.ascontiguousarray(d.vertices).reshape(-1).view(np.uint8)
        idx = np.ascontiguousarray(d.indices).reshape(-1).view(np.uint32)
        if d.index_format != S.R32_UINT or d.stride < VERTEX_BYTES or d.stride % 4 != 0 or ntri > (1 << T):
            stats[1] += ntri
            continue
        t = np.arange(ntri, dtype=np.int64)
        first = d.start_index + 3 * t
        in_ib = first + 2 < idx.size
        tri_idx = idx[np.minimum(first[:, None] + np.arange(3), max(idx.size - 1, 0))].astype(np.int64) if idx.size else np.zeros((ntri, 3), np.int64)
        vi = d.base_vertex + tri_idx
        in_vb = (vi >= 0) & (vi * d.stride + VERTEX_BYTES <= raw.size)
        flat = np.where(in_vb, vi, 0).reshape(-1)
        if raw.size >= VERTEX_BYTES:
            byte = flat[:, None] * d.stride + np.arange(VERTEX_BYTES)
            vert = raw[np.minimum(byte, raw.size - 1)].reshape(-1, VERTEX_BYTES).copy().view(np.float32).reshape(-1, 16)
        else:
            vert = np.zeros((flat.size, 16), np.float32)
        W = np.asarray(d.world, np.float32).reshape(4, 4)
        pos, nrm = vert[:, 0:3], vert[:, 3:6]
        with np.errstate(all="ignore"):
            wv = [((pos[:, 0] * W[0, k] + pos[:, 1] * W[1, k]) + pos[:, 2] * W[2, k]) + W[3, k] for k in range(4)]
            clip = np.stack(D._mul(D._mul(wv, view), proj), axis=1).astype(np.float32).reshape(ntri, 3, 4)
            wn = np.stack([(nrm[:, 0] * W[0, k] + nrm[:, 1] * W[1, k]) + nrm[:, 2] * W[2, k] for k in range(3)], axis=1).astype(np.float32).reshape(ntri, 3, 3)
            wp = np.stack(wv[:3], axis=1).astype(np.float32).reshape(ntri, 3, 3)
            col = vert[:, 12:15].reshape(ntri, 3, 3)
            supported = in_ib & in_vb.all(axis=1) & np.isfinite(clip).all(axis=(1, 2)) & (clip[:, :, 2] > 0).all(axis=1)
        stats[1] += int((~supported).sum())
        keep = np.flatnonzero(supported)
        poly, emit, n_out, B = near_clip(clip[keep])
        stats[4] += int(((n_out == 1) | (n_out == 2)).sum())
        stats[5] += int((n_out == 3).sum())
        X, Y, Z = D.viewport(poly, w, h)
        with np.errstate(all="ignore"):
            bad = ~np.isfinite(X) | ~np.isfinite(Y) | ~np.isfinite(Z) | (np.abs(X) > D.GUARD_BAND) | (np.abs(Y) > D.GUARD_BAND)
        consts = d.constants()
        for k in range(keep.size):
            key = ((o + 1) << T) | int(keep[k])
            for e in range(int(emit[k])):
                u = [0, 2 + e, 1 + e]
                if bad[k, u].any():
                    stats[2] += 1
                    continue
                f = raster(S.snap(X[k, u]), S.snap(Y[k, u]), Z[k, u], w, h)
                if f is None:
                    continue
                stats[0] += 1
                py, px, z, e01, e12, e20 = f
                if not py.size:
                    continue
                frags[(key, e)] = (py * w + px, e01, e12, e20)
                tris[key] = (poly[k, :, 3], B[k], wn[keep[k]], wp[keep[k]], col[keep[k]], consts)
                with np.errstate(all="ignore"):
                    ok = z >= 0
                    zs = np.minimum(z, F1) + np.float32(0.0)
                    if flags & QUANTIZE_D24:
                        zs = D.quantize_d24(zs)
                    ok &= zs >= depth[py, px]
                keys[py[ok], px[ok]] = np.maximum(keys[py[ok], px[ok]], np.uint32(key))

    # ---- the resolve
    flatkeys = keys.reshape(-1)
    at = np.flatnonzero(flatkeys)
    n = at.size
    lam, cw, Br = np.zeros((n, 3), np.int64), np.ones((n, 3), np.float32), np.zeros((n, 3, 3), np.float32)
    wn_, wp_, col_, cs_ = np.zeros((n, 3, 3), np.float32), np.zeros((n, 3, 3), np.float32), np.zeros((n, 3, 3), np.float32), np.zeros((n, CONSTANT_FLOATS), np.float32)
    order = np.argsort(flatkeys[at], kind="stable")
    sorted_keys = flatkeys[at][order]
    bounds = np.flatnonzero(np.r_[True, sorted_keys[1:] != sorted_keys[:-1], True]) if n else np.zeros(1, np.int64)
    for a, b in zip(bounds[:-1], bounds[1:]):
        key = int(sorted_keys[a])
        rows = order[a:b]
        texels = at[rows]
        vw, B, wn, wp, col, consts = tris[key]
        piece = np.ones(texels.size, np.int64)  # emitted triangle 0 if rule 4 covers the centre, else triangle 1
        where = np.zeros(texels.size, np.int64)
        for e in (1, 0):
            if (key, e) in frags:
                f = frags[(key, e)][0]
                srt = np.argsort(f)
                pos = np.clip(np.searchsorted(f[srt], texels), 0, f.size - 1)
                hit = f[srt][pos] == texels
                piece[hit], where[hit] = e, srt[pos][hit]
        for e in (0, 1):
            m = piece == e
            if not m.any():
                continue
            u = [0, 2 + e, 1 + e]
            _, e01, e12, e20 = frags[(key, e)]
            j = where[m]
            lam[rows[m]] = np.stack([e12[j], e20[j], e01[j]], axis=1)
            cw[rows[m]] = vw[u]
            Br[rows[m]] = B[u]
        wn_[rows], wp_[rows], col_[rows], cs_[rows] = wn, wp, col, consts
    A32, albedo32 = shade(lam, cw, Br, wn_, wp_, col_, cs_, view)
    clear_half = np.array([0, 0, 0, 0x3C00], np.uint16)
    out = {k: np.tile(clear_half, (h * w, 1)) for k in ("A", "B", "hdr")}
    out["C"] = np.full(h * w, 0xFF000000, np.uint32)
    out["object_id"] = np.zeros(h * w, np.uint32)
    out["A"][at] = _half(A32)
    out["B"][at] = _half(np.stack([np.full(n, np.float32(0.04)), cs_[:, 104], cs_[:, 105], np.ones(n, np.float32)], axis=1))
    out["hdr"][at] = _half(np.concatenate([cs_[:, 80:83], np.ones((n, 1), np.float32)], axis=1))
    code = srgb_encode(albedo32)
    out["C"][at] = code[:, 0] | (code[:, 1] << 8) | (code[:, 2] << 16) | np.uint32(0xFF000000)
    out["object_id"][at] = cs_.view(np.uint32)[:, 148]
    out = {k: (v.reshape(h, w, 4) if v.ndim == 2 else v.reshape(h, w)) for k, v in out.items()}
    out["keys"], out["stats"] = keys, stats.astype(np.uint32)
    if precise:
        A64, albedo64 = shade(lam, cw, Br, wn_, wp_, col_, cs_, view, np.float64)
        out["covered"], out["A32"], out["A64"], out["code32"], out["albedo64"] = at, A32, A64, code, albedo64
    return out


def accuracy(out):
    """(the largest error of a channel of A in fp16 ulps of the float64 value, the largest difference of a code of C) of a precise run.
    Texels whose float64 value is not finite (a zero normal) are left out: there is no value to measure against."""
    a64 = out["A64"]
    with np.errstate(all="ignore"):
        a16 = out["A32"].astype(np.float16).astype(np.float64)
        ulp = np.exp2(np.floor(np.log2(np.maximum(np.abs(a64), 2.0 ** -14))) - 10)
        err = np.abs(a16 - a64) / ulp
        ok = np.isfinite(a64) & np.isfinite(a16)
        code64 = srgb_encode(out["albedo64"], table().astype(np.float64))
        good = np.isfinite(out["albedo64"])
    worst_a = float(err[ok].max()) if ok.any() else 0.0
    diff = np.abs(out["code32"].astype(np.int64) - code64.astype(np.int64))[good]
    return worst_a, int(diff.max()) if diff.size else 0


def bound(measured: float) -> float:
    """4 x the measured maximum, rounded up to a power of two, never below 1."""
    return max(1.0, float(2.0 ** np.ceil(np.log2(4.0 * measured)))) if measured > 0 else 1.0


# ---- inputs --------------------------------------------------------------------------------------------------------------------------

def soup(w: int, h: int, seed: int, triangles: int = 2000):
    """depth_ref.soup's geometry and draws (its constant-depth triangles that tie at shared texels, its stride-12 draw - unsupported here -,
    its InstanceCount 0, start index, base vertex and World translation) with 64-byte vertices: a seeded normal per triangle with a
    per-vertex perturbation (two triangles get a zero normal at one vertex), seeded colours in [0, 1.25) and per-command constants."""
    rng = np.random.default_rng(seed + 1000)
    out = []
    for k, d in enumerate(D.soup(w, h, seed, triangles)):
        g = GDraw(d.vertices, d.indices, d.world, d.stride, d.index_count, d.instance_count, d.start_index, d.base_vertex, d.index_format,
                  base_color=rng.uniform(0.05, 1.0, 3).astype(np.float32), emissive=rng.uniform(0.0, 4.0, 3).astype(np.float32),
                  metallic=float(np.float32(rng.uniform())), roughness=float(np.float32(rng.uniform(0.05, 1.0))), object_id=int(rng.integers(1, 2 ** 32)))
        if d.stride == VERTEX_BYTES:
            v = np.ascontiguousarray(d.vertices).view(np.float32).reshape(-1, 16).copy()
            nv = v.shape[0]
            base = rng.normal(size=(nv // 3 + 1, 3))
            base /= np.linalg.norm(base, axis=1, keepdims=True)
            v[:, 3:6] = (np.repeat(base, 3, axis=0)[:nv] + 0.3 * rng.normal(size=(nv, 3))).astype(np.float32)
            v[:, 12:15] = rng.uniform(0.0, 1.25, (nv, 3)).astype(np.float32)
            if k == 0:
                v[[10, 50], 3:6] = 0.0
            g.vertices = v.reshape(-1).view(np.uint8).copy()
        out.append(g)
    return out


SOUPS = [(64, 64, 1), (257, 130, 2)]
