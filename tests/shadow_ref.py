"""The ShadowMap raster rule restated in numpy: what ur_shadow_map must compute, to the byte.

Edge functions and the facing test are exact in int64 on the snapped 24.8 coordinates; the fp32 path orders every float operation as
the rule does (numpy float32 arithmetic is IEEE, one rounding per operation, no contraction); the float64 path computes the depth of
the same fragments from the same snapped integers in double precision, for the accuracy bound.

A draw is a Draw: the host copy of what a 64-byte FIndirectDrawCommand slot points at. shadow_map(draws, lvp, w, h) returns the map
and stats[0:3] (rasterised, unsupported, dropped); stats[3] of the kernel is structural (how many large triangles found no room in the
queue) and has no counterpart here.

Depth accuracy, measured by depth_error() over the seeded soups of tests/test_gpu_shadow_map.py (soup(64, 64, 1), soup(257, 130, 2),
soup(2048, 2048, 3)): max |z_fp32 - z_float64| over all covered fragments, before the depth clip = 3.63e-07 = 6.09 x 2^-24 (the 2048^2
soup; 1.79e-07 = 3.01 x 2^-24 on 64 x 64, 2.11e-07 = 3.54 x 2^-24 on 257 x 130). DEPTH_ERROR_BOUND = 32 x 2^-24 = 2^-19 is 4 x that
(24.4 x 2^-24), rounded up to a power of two times 2^-24: the seeds are a sample.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

GUARD_BAND = np.float32(16384.0)
R32_UINT = 42
MEASURED_DEPTH_ERROR = 3.63e-07
DEPTH_ERROR_BOUND = 32.0 * 2.0 ** -24

IDENTITY = np.eye(4, dtype=np.float32).reshape(-1)


@dataclass
class Draw:
    vertices: np.ndarray            # the vertex buffer view's bytes (any dtype; read as raw bytes)
    indices: np.ndarray             # the index buffer view (uint32)
    world: np.ndarray = field(default_factory=lambda: IDENTITY.copy())  # 16 floats, row-major, v' = v @ World
    stride: int = 64
    index_count: "int | None" = None  # default: every index behind start_index
    instance_count: int = 1
    start_index: int = 0
    base_vertex: int = 0
    index_format: int = R32_UINT

    def count(self) -> int:
        return int(self.index_count) if self.index_count is not None else max(int(np.asarray(self.indices).size) - self.start_index, 0)


def vertex_buffer(positions, stride: int = 64, fill: float = 7.0) -> np.ndarray:
    """A vertex buffer of `stride` bytes per vertex with POSITION at byte 0 and a filler in the rest, as raw bytes."""
    p = np.ascontiguousarray(positions, np.float32).reshape(-1, 3)
    v = np.full((p.shape[0], stride // 4), np.float32(fill), np.float32)
    v[:, :3] = p
    return v.reshape(-1).view(np.uint8).copy()


def project(pos: np.ndarray, world: np.ndarray, lvp: np.ndarray) -> np.ndarray:
    """Rule 1: clip = (pos, 1) * World * LightViewProjection, each a left-to-right float32 sum of four products."""
    W = np.asarray(world, np.float32).reshape(4, 4)
    L = np.asarray(lvp, np.float32).reshape(4, 4)
    x, y, z = (pos[:, k].astype(np.float32) for k in range(3))
    with np.errstate(all="ignore"):
        wv = [((x * W[0, k] + y * W[1, k]) + z * W[2, k]) + W[3, k] for k in range(4)]
        clip = [((wv[0] * L[0, k] + wv[1] * L[1, k]) + wv[2] * L[2, k]) + wv[3] * L[3, k] for k in range(4)]
    return np.stack(clip, axis=1).astype(np.float32)


def viewport(clip: np.ndarray, w: int, h: int):
    """Rule 2: X, Y, Z in float32."""
    hw, hh = np.float32(0.5) * np.float32(w), np.float32(0.5) * np.float32(h)
    with np.errstate(all="ignore"):
        X = (clip[:, 0] + np.float32(1.0)) * hw
        Y = (np.float32(1.0) - clip[:, 1]) * hh
    return X.astype(np.float32), Y.astype(np.float32), clip[:, 2].astype(np.float32)


def snap(X: np.ndarray) -> np.ndarray:
    """8 sub-pixel bits, round to nearest even (np.rint is). The caller has excluded non-finite and out-of-band values."""
    return np.rint(np.asarray(X, np.float32) * np.float32(256.0)).astype(np.int64)


def _top_left(dx: int, dy: int) -> bool:
    return dy < 0 or (dy == 0 and dx > 0)


def raster_triangle(xi, yi, z, w: int, h: int, depth: str = "fp32"):
    """Rules 3-5 for one triangle given its snapped coordinates (three ints each) and float32 depths: None when it is culled
    (A <= 0), else (py, px, z) of its fragments BEFORE the depth clip - z float32 ("fp32"), float64 ("fp64"), or both ("both":
    a pair)."""
    x0, x1, x2 = (int(v) for v in xi)
    y0, y1, y2 = (int(v) for v in yi)
    A = (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0)
    if A <= 0:
        return None
    empty = (np.zeros(0, np.int64), np.zeros(0, np.int64), (np.zeros(0, np.float32), np.zeros(0, np.float64)) if depth == "both" else np.zeros(0, np.float32 if depth == "fp32" else np.float64))
    px0, px1 = max(-((128 - min(x0, x1, x2)) // 256), 0), min((max(x0, x1, x2) - 128) // 256, w - 1)
    py0, py1 = max(-((128 - min(y0, y1, y2)) // 256), 0), min((max(y0, y1, y2) - 128) // 256, h - 1)
    if px0 > px1 or py0 > py1:
        return empty
    sx = 256 * np.arange(px0, px1 + 1, dtype=np.int64) + 128
    sy = 256 * np.arange(py0, py1 + 1, dtype=np.int64) + 128
    inside, E = None, []
    for (ax, ay, bx, by) in ((x0, y0, x1, y1), (x1, y1, x2, y2), (x2, y2, x0, y0)):
        dx, dy = bx - ax, by - ay
        e = (dx * (sy - ay))[:, None] - (dy * (sx - ax))[None, :]  # exact: |products| < 2^47
        ok = (e >= 0) if _top_left(dx, dy) else (e > 0)
        inside = ok if inside is None else inside & ok
        E.append(e)
    iy, ix = np.nonzero(inside)
    e01, e20 = E[0][iy, ix], E[2][iy, ix]
    z0, z1, z2 = (np.float32(v) for v in z)
    out = []
    with np.errstate(all="ignore"):
        if depth in ("fp32", "both"):
            inv = np.float32(1.0) / np.float32(A)  # (int -> float32: round to nearest even)
            k1, k2 = (z1 - z0) * inv, (z2 - z0) * inv
            out.append((z0 + (e20.astype(np.float32) * k1 + e01.astype(np.float32) * k2)).astype(np.float32))
        if depth in ("fp64", "both"):
            d0, d1, d2 = float(z0), float(z1), float(z2)
            out.append(d0 + (e20.astype(np.float64) * ((d1 - d0) / A) + e01.astype(np.float64) * ((d2 - d0) / A)))
    return iy + py0, ix + px0, (out[0] if len(out) == 1 else tuple(out))


def _blend(target: np.ndarray, py, px, z):
    """Rule 5's depth clip and +0, rule 6's minimum."""
    keep = (z >= 0) & (z <= 1)  # (false for NaN)
    py, px, z = py[keep], px[keep], z[keep] + z.dtype.type(0.0)
    target[py, px] = np.minimum(target[py, px], z)  # (a triangle's fragments are distinct texels)


def selected_slots(command_count: int, visible=None, index_base: int = 0, ranges=None):
    """The slots a ur_raster_draws selection draws, in no particular order. visible: (visible_idx array, count). ranges: (offsets,
    counts) over the ranges' own command slots."""
    if visible is not None:
        idx, cnt = visible
        k = min(int(cnt), command_count)
        s = (np.asarray(idx, np.uint32)[:k] - np.uint32(index_base)).astype(np.uint32)
        return [int(v) for v in s if v < command_count]
    if ranges is not None:
        offsets, counts = (np.asarray(a, np.int64) for a in ranges)
        out = []
        for r in range(counts.size):
            n = min(int(counts[r]), int(offsets[r + 1] - offsets[r]))
            out += [s for s in range(int(offsets[r]), int(offsets[r]) + n) if s < command_count]
        return out
    return list(range(command_count))


def shadow_map(draws, lvp, w: int, h: int, depth: str = "fp32", slots=None, error_out: "list | None" = None):
    """ur_shadow_map: (map (h, w) float32 - float64 with depth="fp64" -, stats uint32[3]). slots: the selected slots (selected_slots),
    default all. error_out: a list that receives max |z_fp32 - z_float64| over the covered fragments of every triangle."""
    dt = np.float64 if depth == "fp64" else np.float32
    target = np.ones((h, w), dt)
    stats = np.zeros(3, np.int64)
    for s in (range(len(draws)) if slots is None else slots):
        d = draws[s]
        if d.instance_count == 0:
            continue
        ntri = d.count() // 3
        raw = np.ascontiguousarray(d.vertices).reshape(-1).view(np.uint8)
        idx = np.ascontiguousarray(d.indices).reshape(-1).view(np.uint32)
        if d.index_format != R32_UINT or d.stride < 12 or d.stride % 4 != 0:
            stats[1] += ntri
            continue
        t = np.arange(ntri, dtype=np.int64)
        first = d.start_index + 3 * t
        in_ib = first + 2 < idx.size
        tri_idx = idx[np.minimum(first[:, None] + np.arange(3), max(idx.size - 1, 0))].astype(np.int64) if idx.size else np.zeros((ntri, 3), np.int64)
        vi = d.base_vertex + tri_idx
        in_vb = (vi >= 0) & (vi * d.stride + 12 <= raw.size)
        flat = np.where(in_vb, vi, 0).reshape(-1)
        if raw.size >= 12:
            byte = flat[:, None] * d.stride + np.arange(12)
            pos = raw[np.minimum(byte, raw.size - 1)].reshape(-1, 12).copy().view(np.float32).reshape(-1, 3)
        else:
            pos = np.zeros((flat.size, 3), np.float32)
        clip = project(pos, d.world, lvp)
        X, Y, Z = viewport(clip, w, h)
        X, Y, Z, cw = (a.reshape(ntri, 3) for a in (X, Y, Z, clip[:, 3]))
        unsupported = ~in_ib | ~in_vb.all(axis=1) | (cw != np.float32(1.0)).any(axis=1)
        with np.errstate(all="ignore"):
            bad = ~np.isfinite(X) | ~np.isfinite(Y) | ~np.isfinite(Z) | (np.abs(X) > GUARD_BAND) | (np.abs(Y) > GUARD_BAND)
        dropped = ~unsupported & bad.any(axis=1)
        stats[1] += int(unsupported.sum())
        stats[2] += int(dropped.sum())
        for k in np.flatnonzero(~unsupported & ~dropped):
            frag = raster_triangle(snap(X[k]), snap(Y[k]), Z[k], w, h, "both" if error_out is not None else depth)
            if frag is None:
                continue
            stats[0] += 1
            py, px, z = frag
            if error_out is not None:
                z32, z64 = z
                if z32.size:
                    error_out.append(float(np.max(np.abs(z32.astype(np.float64) - z64))))
                z = z64 if depth == "fp64" else z32
            _blend(target, py, px, z)
    return target, stats.astype(np.uint32)


def depth_error(draws, lvp, w: int, h: int) -> float:
    """max |z_fp32 - z_float64| over every covered fragment (before the depth clip) of the draws."""
    errs = []
    shadow_map(draws, lvp, w, h, error_out=errs)
    return max(errs) if errs else 0.0


# ---- inputs in target space -------------------------------------------------------------------------------------------------------

def target_lvp() -> np.ndarray:
    """The identity: positions are clip coordinates."""
    return IDENTITY.copy()


def target_to_clip(X, Y, Z, w: int, h: int) -> np.ndarray:
    """Positions whose rule-2 coordinates are (X, Y, Z) under identity matrices: exactly so when w and h are powers of two and X, Y
    are multiples of 2^-10 (every operation is exact), within an ulp otherwise."""
    X, Y, Z = (np.asarray(a, np.float64) for a in (X, Y, Z))
    return np.stack([X / (0.5 * w) - 1.0, 1.0 - Y / (0.5 * h), Z], axis=-1).astype(np.float32)


def soup(w: int, h: int, seed: int, triangles: int = 2000):
    """The seeded triangle soup of the GPU test: `triangles` triangles in five draws. Edge lengths are log-uniform from 1/8 px to twice
    the target; half the vertices sit on the half-pixel lattice (pixel centres and pixel corners), so edges and vertices hit centres;
    windings are mixed; depth runs over [-0.2, 1.2]. Draw 1 has InstanceCount = 0, draw 2 a non-zero StartIndexLocation and
    BaseVertexLocation, draw 3 a vertex stride of 12, draw 4 a World translation (undone in its positions up to rounding)."""
    rng = np.random.default_rng(seed)
    size = float(max(w, h))
    n = triangles
    centre = np.stack([rng.uniform(-0.05 * w, 1.05 * w, n), rng.uniform(-0.05 * h, 1.05 * h, n)], axis=1)
    length = np.exp(rng.uniform(np.log(0.125), np.log(2.0 * size), n))
    P = centre[:, None, :] + rng.uniform(-0.5, 0.5, (n, 3, 2)) * length[:, None, None]
    lattice = rng.random((n, 3)) < 0.5
    P = np.where(lattice[..., None], np.round(P * 2.0) / 2.0, P)
    Zs = rng.uniform(-0.2, 1.2, (n, 3))
    flat = rng.random(n) < 0.1  # some constant-depth triangles: equal depths meet at shared texels
    Zs = np.where(flat[:, None], np.round(Zs[:, :1] * 8.0) / 8.0, Zs)
    pos = target_to_clip(P[..., 0], P[..., 1], Zs, w, h)  # (n, 3, 3)
    bounds = [0, n // 5, 2 * n // 5, 3 * n // 5, 4 * n // 5, n]
    draws = []
    for k in range(5):
        p = pos[bounds[k]:bounds[k + 1]].reshape(-1, 3)
        idx = rng.permutation(p.shape[0] // 3)[:, None] * 3 + np.arange(3)  # triangles in a shuffled order, vertices in theirs
        idx = idx.reshape(-1).astype(np.uint32)
        d = Draw(vertex_buffer(p), idx)
        if k == 1:
            d.instance_count = 0
        elif k == 2:  # 5 unused vertices in front (BaseVertexLocation), 7 unused indices in front (StartIndexLocation), 2 behind
            d.vertices = vertex_buffer(np.concatenate([np.full((5, 3), 0.25, np.float32), p]))
            d.indices = np.concatenate([np.zeros(7, np.uint32), idx, np.array([1, 2], np.uint32)])
            d.start_index, d.base_vertex, d.index_count = 7, 5, idx.size + 2
        elif k == 3:
            d.vertices, d.stride = vertex_buffer(p, 12), 12
        elif k == 4:
            t = np.array([0.375, -0.25, 0.0625], np.float32)
            d.world = np.eye(4, dtype=np.float32)
            d.world[3, :3] = t
            d.world = d.world.reshape(-1)
            d.vertices = vertex_buffer(p - t)
        draws.append(d)
    return draws
