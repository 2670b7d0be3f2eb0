"""The DepthPrepass raster rule restated in numpy: what ur_depth_prepass must compute, to the byte.

The draws, their selections and their command, index and vertex checks are tests/shadow_ref.py's (section 3.7); so are coverage and the
depth plane (raster_triangle), which this file calls with every emitted triangle (u0, u1, u2) reordered to (u0, u2, u1). New here: the
three matrix products, the near clip, the divide, the 2^21 px guard band, the clamp at 1, the per-texel maximum and the D24 quantiser.
numpy float32 arithmetic is IEEE, one rounding per operation, no contraction, division included.

depth_prepass(draws, view, projection, w, h) returns the target and stats[0:6] as the kernel counts them; stats[3] (large triangles that
found no room in the queue) is structural and stays 0 here.

Depth accuracy, measured by depth_error() over the seeded soups of tests/test_gpu_depth_prepass.py (SOUPS below): max |z_fp32 -
z_float64| over all covered fragments, before the clamp, the float64 value from the same snapped integers and per-vertex depths =
1.56e-07 = 2.61 x 2^-24 (the 1024 x 512 soup; 1.26e-07 = 2.11 x 2^-24 on 64 x 64, 1.24e-07 = 2.09 x 2^-24 on 257 x 130).
DEPTH_ERROR_BOUND = 16 x 2^-24 = 2^-20 is 4 x that (10.4 x 2^-24), rounded up to a power of two: the seeds are a sample.
"""
from __future__ import annotations

import numpy as np

from tests import shadow_ref as S
from tests.shadow_ref import Draw, vertex_buffer, selected_slots  # noqa: F401  (the draws are section 3.7's)

GUARD_BAND = np.float32(2097152.0)  # 2^21 px
QUANTIZE_D24 = 0x1
MEASURED_DEPTH_ERROR = 1.56e-07
DEPTH_ERROR_BOUND = 16.0 * 2.0 ** -24

IDENTITY = S.IDENTITY
F1, F0 = np.float32(1.0), np.float32(0.0)


def projection(near: float, w: int, h: int, fov_y: float = np.pi / 4) -> np.ndarray:
    """The reference's reverse-Z projection with an infinite far plane (Camera.cpp:41-46), row-vector convention: clip.z = near *
    view.w, clip.w = view.z."""
    ys = 1.0 / np.tan(0.5 * fov_y)
    xs = ys * h / w
    return np.array([xs, 0, 0, 0, 0, ys, 0, 0, 0, 0, 0, 1, 0, 0, near, 0], np.float32)


def _mul(v, M):
    """Row vector times a 4 x 4 matrix: for every column the left-to-right float32 sum of four products."""
    M = np.asarray(M, np.float32).reshape(4, 4)
    return [((v[0] * M[0, k] + v[1] * M[1, k]) + v[2] * M[2, k]) + v[3] * M[3, k] for k in range(4)]


def project(pos: np.ndarray, world, view, proj) -> np.ndarray:
    """Vertex rule: clip = ((pos, 1) * World) * View) * Projection, never a pre-multiplied matrix."""
    W = np.asarray(world, np.float32).reshape(4, 4)
    x, y, z = (pos[:, k].astype(np.float32) for k in range(3))
    with np.errstate(all="ignore"):
        wv = [((x * W[0, k] + y * W[1, k]) + z * W[2, k]) + W[3, k] for k in range(4)]
        clip = _mul(_mul(wv, view), proj)
    return np.stack(clip, axis=1).astype(np.float32)


def near_clip(c: np.ndarray):
    """c: (n, 3, 4) clip-space triangles, every coordinate finite, z > 0. Returns (S (n, 4, 4) polygon vertices in clip space, emit (n,)
    0 / 1 / 2, n_out (n,)): emitted triangle e of a polygon is (S0, S[1 + e], S[2 + e])."""
    with np.errstate(all="ignore"):
        d = (c[:, :, 3] - c[:, :, 2]).astype(np.float32)
        out = d < 0
        n_out = out.sum(axis=1)
        # (a, b, c): rotated, winding kept, so that c is the one vertex outside, or a the one vertex inside
        rot = np.where(n_out == 1, np.where(out[:, 0], 1, np.where(out[:, 1], 2, 0)),
                       np.where(n_out == 2, np.where(~out[:, 0], 0, np.where(~out[:, 1], 1, 2)), 0))
        rows = np.arange(c.shape[0])
        a, b, cc = (c[rows, (rot + k) % 3] for k in range(3))
        da, db, dc = (d[rows, (rot + k) % 3] for k in range(3))
        one, two, whole = (n_out == 1)[:, None], (n_out == 2)[:, None], (n_out == 0)[:, None]

        def cut(i, o, di, do):  # from the inside vertex towards the outside one; z := w
            t = (di / (di - do)).astype(np.float32)[:, None]
            v = (i + t * (o - i)).astype(np.float32)
            v[:, 2] = v[:, 3]
            return v

        p = cut(np.where(one, b, a), np.where(one, cc, b), np.where(one[:, 0], db, da), np.where(one[:, 0], dc, db))
        q = cut(a, cc, da, dc)
        poly = np.stack([a, np.where(two, p, b), np.where(whole, cc, np.where(one, p, q)), q], axis=1)
    emit = np.where(n_out == 3, 0, np.where(n_out == 1, 2, 1))
    return poly.astype(np.float32), emit, n_out


def viewport(poly: np.ndarray, w: int, h: int):
    """X = (cx / cw + 1) * (0.5 w), Y = (1 - cy / cw) * (0.5 h), Z = cz / cw, IEEE divisions."""
    hw, hh = np.float32(0.5) * np.float32(w), np.float32(0.5) * np.float32(h)
    with np.errstate(all="ignore"):
        cw = poly[..., 3]
        X = (poly[..., 0] / cw + F1) * hw
        Y = (F1 - poly[..., 1] / cw) * hh
        Z = poly[..., 2] / cw
    return X.astype(np.float32), Y.astype(np.float32), Z.astype(np.float32)


def quantize_d24(z: np.ndarray) -> np.ndarray:
    """(float)(rint((double)z * 16777215.0) / 16777215.0): the bytes of synth.quantize_d24."""
    return (np.rint(z.astype(np.float64) * 16777215.0) / 16777215.0).astype(np.float32)


def triangle_class(xi, yi, w: int, h: int) -> str:
    """How the kernel serves a drawn triangle, from its bounding box clamped to the target: "none" (no centre under it), "own" (at most
    4 centres), "wave" (at most 64 8 x 8 stamps) or "large"."""
    bx0, bx1 = max((int(min(xi)) + 127) >> 8, 0), min((int(max(xi)) - 128) >> 8, w - 1)
    by0, by1 = max((int(min(yi)) + 127) >> 8, 0), min((int(max(yi)) - 128) >> 8, h - 1)
    if bx0 > bx1 or by0 > by1:
        return "none"
    if (bx1 - bx0 + 1) * (by1 - by0 + 1) <= 4:
        return "own"
    return "wave" if ((bx1 >> 3) - (bx0 >> 3) + 1) * ((by1 >> 3) - (by0 >> 3) + 1) <= 64 else "large"


def depth_prepass(draws, view, proj, w: int, h: int, flags: int = 0, slots=None, depth: str = "fp32", error_out: "list | None" = None,
                  info: "dict | None" = None):
    """ur_depth_prepass: (target (h, w) float32 - float64 with depth="fp64" -, stats uint32[6]). slots: the selected slots, default all.
    error_out: receives max |z_fp32 - z_float64| over the covered fragments of every drawn triangle. info: receives the counts "one_out",
    "two_out" and the triangle classes "own", "wave", "large", "none"."""
    dt = np.float64 if depth == "fp64" else np.float32
    target = np.zeros((h, w), dt)
    stats = np.zeros(6, np.int64)
    if info is not None:
        info.update({k: info.get(k, 0) for k in ("one_out", "two_out", "own", "wave", "large", "none")})
    for s in (range(len(draws)) if slots is None else slots):
        d = draws[s]
        if d.instance_count == 0:
            continue
        ntri = d.count() // 3
        raw = np.ascontiguousarray(d.vertices).reshape(-1).view(np.uint8)
        idx = np.ascontiguousarray(d.indices).reshape(-1).view(np.uint32)
        if d.index_format != S.R32_UINT or d.stride < 12 or d.stride % 4 != 0:
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
        clip = project(pos, d.world, view, proj).reshape(ntri, 3, 4)
        with np.errstate(all="ignore"):
            supported = in_ib & in_vb.all(axis=1) & np.isfinite(clip).all(axis=(1, 2)) & (clip[:, :, 2] > 0).all(axis=1)
        stats[1] += int((~supported).sum())
        keep = np.flatnonzero(supported)
        poly, emit, n_out = near_clip(clip[keep])
        stats[4] += int(((n_out == 1) | (n_out == 2)).sum())
        stats[5] += int((n_out == 3).sum())
        if info is not None:
            info["one_out"] += int((n_out == 1).sum())
            info["two_out"] += int((n_out == 2).sum())
        X, Y, Z = viewport(poly, w, h)
        with np.errstate(all="ignore"):
            bad = ~np.isfinite(X) | ~np.isfinite(Y) | ~np.isfinite(Z) | (np.abs(X) > GUARD_BAND) | (np.abs(Y) > GUARD_BAND)
        for k in range(keep.size):
            for e in range(int(emit[k])):
                u = [0, 2 + e, 1 + e]  # (u0, u2, u1): drawn iff A > 0 of the reordered triangle, A < 0 of the emitted one
                if bad[k, u].any():
                    stats[2] += 1
                    continue
                xi, yi = S.snap(X[k, u]), S.snap(Y[k, u])
                frag = S.raster_triangle(xi, yi, Z[k, u], w, h, "both" if error_out is not None else depth)
                if frag is None:
                    continue
                stats[0] += 1
                if info is not None:
                    info[triangle_class(xi, yi, w, h)] += 1
                py, px, z = frag
                if error_out is not None:
                    z32, z64 = z
                    if z32.size:
                        error_out.append(float(np.max(np.abs(z32.astype(np.float64) - z64))))
                    z = z64 if depth == "fp64" else z32
                with np.errstate(all="ignore"):
                    ok = z >= 0  # (false for NaN)
                py, px, z = py[ok], px[ok], np.minimum(z[ok], z.dtype.type(1.0)) + z.dtype.type(0.0)
                if flags & QUANTIZE_D24:
                    z = quantize_d24(z).astype(dt)
                target[py, px] = np.maximum(target[py, px], z)  # (a triangle's fragments are distinct texels)
    return target, stats.astype(np.uint32)


def depth_error(draws, view, proj, w: int, h: int) -> float:
    errs = []
    depth_prepass(draws, view, proj, w, h, error_out=errs)
    return max(errs) if errs else 0.0


# ---- inputs --------------------------------------------------------------------------------------------------------------------------

NEAR = 0.125


def hand_camera(w: int, h: int):
    """View = identity and a projection under which the position (x, y, z) has clip (x, y, NEAR, z): with w, h powers of two a vertex
    (X, Y) on the target at view depth z = 2^k is exact in every operation."""
    return IDENTITY.copy(), np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, NEAR, 0], np.float32)


def at(X, Y, z, w: int, h: int):
    """The view-space position that hand_camera puts at target (X, Y) with view depth z (target depth NEAR / z)."""
    return [(X / (0.5 * w) - 1.0) * z, (1.0 - Y / (0.5 * h)) * z, z]


def soup_camera(w: int, h: int):
    """A camera off the axes: a rotation about y, a translation, the reference's projection."""
    c, s = np.cos(0.3), np.sin(0.3)
    view = np.array([c, 0, s, 0, 0, 1, 0, 0, -s, 0, c, 0, 0.25, -0.5, 1.5, 1], np.float64)
    return view.astype(np.float32), projection(NEAR, w, h)


def soup(w: int, h: int, seed: int, triangles: int = 2000, dirty: bool = False):
    """The seeded soup of the GPU test under soup_camera(w, h): five draws shaped like section 3.7's soup (InstanceCount 0, a start index
    and base vertex, a stride of 12, a World translation). 60 % of the triangles lie in front of the near plane - edge lengths log-uniform
    from 1/8 px to twice the target, half the vertices on the half-pixel lattice before the matrices round them -, 30 % have one or two
    vertices pushed behind the near plane (some behind the eye), 10 % lie wholly behind it. dirty: a sixth draw of 30 triangles with a NaN
    or overflowing vertex and 30 with a vertex in front of the near plane but far outside the guard band."""
    rng = np.random.default_rng(seed)
    view, proj = soup_camera(w, h)
    xs, ys = float(proj[0]), float(proj[5])
    size = float(max(w, h))
    n = triangles
    kind = rng.choice(3, n, p=[0.6, 0.3, 0.1])  # 0 in front, 1 crossing, 2 behind
    centre = np.stack([rng.uniform(-0.05 * w, 1.05 * w, n), rng.uniform(-0.05 * h, 1.05 * h, n)], axis=1)
    length = np.exp(rng.uniform(np.log(0.125), np.log(2.0 * size), n))
    length = np.where(kind == 1, np.clip(length, 1.0, size), length)
    P = centre[:, None, :] + rng.uniform(-0.5, 0.5, (n, 3, 2)) * length[:, None, None]
    lattice = rng.random((n, 3)) < 0.5
    P = np.where(lattice[..., None], np.round(P * 2.0) / 2.0, P)
    zc = np.where(kind == 0, np.exp(rng.uniform(np.log(1.2 * NEAR), np.log(200.0 * NEAR), n)), rng.uniform(1.2 * NEAR, 4.0 * NEAR, n))
    zv = zc[:, None] * np.exp(rng.uniform(-0.15, 0.15, (n, 3)))
    flat = rng.random(n) < 0.1  # some constant-depth triangles: equal depths meet at shared texels
    zv = np.where(flat[:, None], zc[:, None], zv)
    vx = (P[..., 0] / (0.5 * w) - 1.0) * zv / xs
    vy = (1.0 - P[..., 1] / (0.5 * h)) * zv / ys
    # crossing: one or two vertices behind the near plane (their x, y stay); behind: all three
    pushed = rng.uniform(-1.5 * NEAR, 0.9 * NEAR, (n, 3))
    n_push = np.where(kind == 1, rng.integers(1, 3, n), np.where(kind == 2, 3, 0))
    order = np.argsort(rng.random((n, 3)), axis=1)
    push = order < n_push[:, None]
    vz = np.where(push, pushed, zv)
    pv = np.stack([vx, vy, vz, np.ones_like(vx)], axis=-1)  # view space
    inv = np.linalg.inv(view.astype(np.float64).reshape(4, 4))
    pos = (pv @ inv)[..., :3].astype(np.float32)  # World = identity
    bounds = [0, n // 5, 2 * n // 5, 3 * n // 5, 4 * n // 5, n]
    draws = []
    for k in range(5):
        p = pos[bounds[k]:bounds[k + 1]].reshape(-1, 3)
        idx = (rng.permutation(p.shape[0] // 3)[:, None] * 3 + np.arange(3)).reshape(-1).astype(np.uint32)
        d = Draw(vertex_buffer(p), idx)
        if k == 1:
            d.instance_count = 0
        elif k == 2:
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
    if dirty:
        m = 30
        good = pos[kind == 0][:2 * m].copy()  # in front
        broken = good[:m].copy()
        broken[np.arange(m), rng.integers(0, 3, m)] = np.array([[np.nan, 0, 0], [3.0e38, 3.0e38, 1.0], [0, np.inf, 0]], np.float32)[rng.integers(0, 3, m)]
        far = np.stack([rng.choice([-1.0, 1.0], m) * np.exp(rng.uniform(np.log(1e5), np.log(1e7), m)) * NEAR / xs, rng.uniform(-1, 1, m),
                        np.full(m, 1.01 * NEAR), np.ones(m)], axis=-1)
        outside = good[m:2 * m].copy()
        outside[np.arange(m), rng.integers(0, 3, m)] = (far @ inv)[:, :3].astype(np.float32)
        p = np.concatenate([broken, outside]).reshape(-1, 3)
        draws.append(Draw(vertex_buffer(p), np.arange(p.shape[0], dtype=np.uint32)))
    return draws


# (w, h, seed) of the GPU test's soups; tests/test_depth_ref.py asserts the soup conditions on them
SOUPS = [(64, 64, 1), (257, 130, 2), (1024, 512, 3)]
DIRTY_SEED = 11
