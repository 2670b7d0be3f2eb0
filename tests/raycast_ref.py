"""A float64 ray caster over the raster passes' draws: the independent check of ShadowMap, DepthPrepass and GBuffer.

The restatements (tests/shadow_ref.py, depth_ref.py, gbuffer_ref.py) and the kernels were written from one rule text, so a mistake in the
rule is invisible between them. This file shares no step with that rule: it does not snap, has no edge functions, no clip polygon and no
barycentrics in screen space. From the restatements it imports only the draw records (Draw, GDraw) and gbuffer_ref.vertex_buffer. It sends
a ray through every texel centre (px + 0.5, py + 0.5), intersects it with every triangle of every draw in world space, and evaluates the
winner's attributes with world-space barycentrics.

Conventions, each worked out from the API state DESIGN.md names and not from the rule's formulas:
  * row vectors: clip = (p, 1) . World . View . Projection; a texel centre (X, Y) has NDC (X / (w/2) - 1, 1 - Y / (h/2)) (y up in NDC,
    down on the target); a ray is the pre-image of that NDC point under the float64 inverse of View . Projection (LightViewProjection).
  * facing: D3D's FrontCounterClockwise calls a triangle front when it is counter-clockwise as seen on the target. The matrices are
    left-handed without a mirror (x right, y up, z into the screen), so a triangle seen counter-clockwise has its geometric normal
    n = (v1 - v0) x (v2 - v0) pointing away from the viewer: front iff n . d > 0 for the ray direction d. The camera passes cull back
    faces (CULL_MODE_BACK: keep n . d > 0), ShadowMap culls front faces (CULL_MODE_FRONT: keep n . d < 0).
  * near plane: a hit counts when its clip coordinates have w > 0 and z <= w - for the reverse-Z projection (z = near, w = view z) that is
    a view depth beyond `near`. This test of the hit point is all there is in place of the near clip. ShadowMap keeps hits with depth in
    [0, 1].
  * winner: the largest z / w under the camera (reverse-Z), the smallest under the light.
  * the normal goes through World's upper 3 x 3 as the vertex shader does (mul(N, (float3x3)World)) - NOT through the inverse transpose,
    which a non-uniform scale would call for; it is then normalised, taken through View's 3 x 3 and normalised again.
  * view depth = -((hit, 1) . View).z, the sign DESIGN.md 3.9 and the shader give it: negative in front of this left-handed camera.

Which texels are compared. Besides the centre, 8 rays go through (px + 0.5 +- DELTA, py + 0.5 +- DELTA) and the four axis offsets. A
texel is compared when all 9 rays hit or all 9 miss, all hits are of one draw, every triangle the rays hit has a smallest screen-space
altitude of at least 1 px, and the 9 view depths spread by at most 4 x what the centre triangle's own plane gives under the same 9 rays.
Every other texel is left out; at most LEFT_OUT_CAP of the texels any ray hits may be. Edges shared inside a mesh are compared.
The tolerance of a value at a compared texel is the spread (max - min) of the ray caster's own value over the 9 rays plus the project's
fp32 bound for that output (S.DEPTH_ERROR_BOUND, D.DEPTH_ERROR_BOUND, A_ULPS_BOUND fp16 ulps, C_CODES_BOUND codes between the encoded
ends of the spread); ObjectId, B, the HDR start value and "covered or clear" are exact.

Measured margins, restatement against ray caster, largest error / tolerance over the compared texels (tests/test_raycast_ref.py records
them per scene and target with record_property and asserts each is at most 1). The kernels on an MI355X give the same figures.
  scene              left out (64 x 64, 257 x 130)   depth            A                C
  icosphere          3.55 %, 0.54 %                  0.0279, 0.0263   0.1193, 0.1225   0.5, 0.5
  torus              1.99 %, 0.55 %                  0.0261, 0.0295   0.1219, 0.1233   0.5, 0.5
  near-plane strip   1.15 %, 0.55 %                  0.0245, 0.0278   0.1248, 0.1250   0.5, 0.5
  two draws          2.16 %, 0.64 %                  0.0268, 0.0295   0.1219, 0.1233   0.5, 0.5  (either order)
  shadow             3.69 %, 1.31 %                  0.0278, 0.0379   -                -
A's 0.125 is the half ulp of fp16 rounding over the 4-ulp bound, C's 0.5 one code where the spread's ends encode alike; ObjectId, B, HDR
and covered-or-clear agree exactly everywhere. No disagreement was found, so no rule changed.

The textured, the alpha-masked and the forward pass are held by tests/raycast_tex.py, which takes hits() - every
hit of every ray with the whole 64-byte vertex - and winners() from here and adds the pixel shaders' material, the alpha test and the
level of detail. Its scenes against the section 3.10 bounds (128 fp16 ulps, 4 codes), the same way; its docstring has every output:
  scene              left out (64 x 64, 257 x 130)   A                C          B.yz             hdr (emissive)
  textured           1.86 %, 0.28 %                  0.0255, 0.0253   0.2, 0.2   0.0041, 0.0041   0.0041, 0.0040
  textured strip     1.15 %, 0.55 %                  0.0163, 0.0249   0.2, 0.2   0.0045, 0.0047   0.0042, 0.0049
  levels             3.70 %, 2.74 %                  0.0093, 0.0165   0.2, 0.2   0.4476, 0.4525   0.4436, 0.4526  (the level read back: 0.4734, 0.4746)
  masked             1.27 %, 0.28 %                  0.0225, 0.0238   0.2, 0.2   0.0041, 0.0041   0.0040, 0.0040  (depth behind the pass: 0.0242, 0.0247)
  forward            4.39 %, 0.99 % (textured), 2.69 %, 0.65 % (masked); hdr within 0.2383, 0.2456 and 0.2368, 0.2436 of 2 fp16 ulps + spread
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from tests.gbuffer_ref import GDraw, vertex_buffer
from tests.shadow_ref import Draw  # noqa: F401  (GDraw's base: the record ShadowMap takes)

# The rule snaps a vertex to 1/256 px, so it moves by at most sqrt(2)/512 px = 0.00276 px. DELTA = 1/32 px is 11.3 x that: the 8 outer
# rays bracket every texel centre as seen from the snapped triangle.
DELTA = 1.0 / 32.0
OFFSETS = np.array([(0, 0), (-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (1, -1), (-1, 1), (1, 1)], np.float64) * DELTA
MIN_ALTITUDE_PX = 1.0
SHEET_FACTOR = 4.0
LEFT_OUT_CAP = 0.05
TARGETS = [(64, 64), (257, 130)]
_ROUNDING = 1e-9  # float64 rounding of the ray caster itself, relative: lets two coplanar triangles pass the sheet test


# ---- the draws as triangles -----------------------------------------------------------------------------------------------------------

def _mesh(d):
    """Every attribute of a draw's triangles in float64, object space: (positions (n, 3, 3), normals (n, 3, 3), colours (n, 3, 4) with
    COLOR.a, texcoords (n, 3, 2), tangents (n, 3, 4) with TANGENT.w). A vertex shorter than 64 bytes has position alone."""
    if d.instance_count == 0:
        return np.zeros((0, 3, 3)), np.zeros((0, 3, 3)), np.zeros((0, 3, 4)), np.zeros((0, 3, 2)), np.zeros((0, 3, 4))
    raw = np.ascontiguousarray(d.vertices).reshape(-1).view(np.uint8)
    floats = raw[:raw.size // d.stride * d.stride].reshape(-1, d.stride)
    idx = np.ascontiguousarray(d.indices).reshape(-1).view(np.uint32).astype(np.int64)
    n = d.count() // 3
    tri = idx[d.start_index:d.start_index + 3 * n].reshape(n, 3) + d.base_vertex
    v = floats[tri.reshape(-1)].copy().view(np.float32).astype(np.float64).reshape(n, 3, -1)
    if v.shape[2] >= 16:
        return v[:, :, 0:3], v[:, :, 3:6], v[:, :, 12:16], v[:, :, 6:8], v[:, :, 8:12]
    return v[:, :, 0:3], np.zeros((n, 3, 3)), np.ones((n, 3, 4)), np.zeros((n, 3, 2)), np.zeros((n, 3, 4))


def _m4(m):
    return np.asarray(m, np.float32).astype(np.float64).reshape(4, 4)


# ---- the cast -------------------------------------------------------------------------------------------------------------------------

def _rays(X, Y, w, h, inv_vp, light):
    """Origins and directions (n, 3) of the rays through the target positions (X, Y): the pre-images of NDC depth 1 -> 0.5 under the
    camera (the origin lies on the near plane), 0 -> 1 under the light."""
    ndc = np.stack([np.ravel(X) / (0.5 * w) - 1.0, 1.0 - np.ravel(Y) / (0.5 * h)], axis=-1)

    def back(z):
        p = np.concatenate([ndc, np.full((ndc.shape[0], 1), z), np.ones((ndc.shape[0], 1))], axis=1) @ inv_vp
        return p[:, :3] / p[:, 3:4]

    a, b = (back(0.0), back(1.0)) if light else (back(1.0), back(0.5))
    return a, b - a


def _lines(o, d):
    """Pluecker coordinates (d, o x d) of rays."""
    return np.concatenate([d, np.cross(o, d)], axis=1)


def cast(draws, w: int, h: int, view=None, proj=None, lvp=None, tile: int = 16):
    """Cast the 9 rays of every texel. Camera: view and proj; light: lvp. Returns a dict of arrays whose first axes are (9, h, w):
    hit (bool), draw and tri (int, -1 on a miss; tri counts the draw's triangles), depth (z / w), view_depth, normal (.., 3), albedo
    (.., 3) - NaN on a miss -, and, for classify(), "gtri" (the triangle counted over all draws), "altitude" (per such triangle: its
    smallest screen-space altitude in px) and "plane_spread" ((h, w): the sheet test's prediction). tile: see below; any value gives
    the same result."""
    H = hits(draws, w, h, view, proj, lvp, tile)
    order = np.lexsort((H["z"] if H["light"] else -H["z"], H["ray"]))  # per ray, the winner first
    first = order[np.r_[True, H["ray"][order][1:] != H["ray"][order][:-1]]] if order.size else order
    return winners(H, first)


def hits(draws, w: int, h: int, view=None, proj=None, lvp=None, tile: int = 16):
    """Every hit of every ray, not only the nearest: a dict of the rays (o, d (9 h w, 3)), the triangles in world space (P, and per
    vertex N, C (rgba), UV, TAN: the tangent through World's 3 x 3, normalised per vertex as the vertex shaders do, with w passed
    through; owner, local), and per hit its ray, triangle (counted over all draws), world-space barycentrics, point and depth z / w."""
    light = lvp is not None
    V = None if light else _m4(view)
    VP = _m4(lvp) if light else V @ _m4(proj)
    along = VP[:, 2] if light else V[:, 2]  # "view depth" = -(p . along): under the light its depth stands in (for the sheet test only)
    inv_vp = np.linalg.inv(VP)
    py, px = np.mgrid[0:h, 0:w]
    o, d = _rays(px[None] + 0.5 + OFFSETS[:, 0, None, None], py[None] + 0.5 + OFFSETS[:, 1, None, None], w, h, inv_vp, light)
    R = o.shape[0]

    P, N, C, UV, TAN, owner, local, base = [], [], [], [], [], [], [], []
    for k, dr in enumerate(draws):
        p, n, c, uv, tan = _mesh(dr)
        W = _m4(dr.world)
        P.append(p @ W[:3, :3] + W[3, :3])
        N.append(n @ W[:3, :3])  # the shader's mul(N, (float3x3)World)
        C.append(c)
        UV.append(uv)
        with np.errstate(all="ignore"):
            t = tan[:, :, :3] @ W[:3, :3]
            TAN.append(np.concatenate([t / np.linalg.norm(t, axis=2, keepdims=True), tan[:, :, 3:4]], axis=2))
        owner.append(np.full(p.shape[0], k))
        local.append(np.arange(p.shape[0]))
        base.append(np.asarray(getattr(dr, "base_color", np.ones(3)), np.float64))
    P, N, C, UV, TAN, owner, local = (np.concatenate(a) for a in (P, N, C, UV, TAN, owner, local))
    T = P.shape[0]

    # Pluecker side products: for the edge v_i -> v_j, u = d . (v_i x v_j) + (v_j - v_i) . (o x d) = d . ((v_i - o) x (v_j - o)). The three
    # of a triangle sum to d . n and are its barycentric numerators: the weight of vertex k is u_k / sum for the edge opposite k.
    vi, vj = P[:, [1, 2, 0]], P[:, [2, 0, 1]]
    edges = np.concatenate([np.cross(vi, vj), vj - vi], axis=2).reshape(T * 3, 6)
    keep_sign = -1.0 if light else 1.0

    # Tiles of texels, for speed alone. Along a ray and under a positive scale of d the sign of u does not change, and with the origin
    # taken at the eye (at infinity under the light) u is affine in the target position: an edge with u < 0 at the four corner rays of a
    # tile (the offsets included) has u < 0 on all of it, and so has the sum d . n. Such triangles are skipped; nothing else is.
    hr, ht, hb = [], [], []
    ray_index = np.arange(R).reshape(9, h, w)
    for y0 in range(0, h, tile):
        for x0 in range(0, w, tile):
            y1, x1 = min(y0 + tile, h), min(x0 + tile, w)
            cx, cy = np.array([x0 + 0.5 - DELTA, x1 - 0.5 + DELTA]), np.array([y0 + 0.5 - DELTA, y1 - 0.5 + DELTA])
            co, cd = _rays(*np.meshgrid(cx, cy), w, h, inv_vp, light)
            Uc = (_lines(co, cd) @ edges.T).reshape(4, T, 3) * keep_sign
            alive = np.flatnonzero(~((Uc < 0).all(axis=0).any(axis=1) | (Uc.sum(axis=2) <= 0).all(axis=0)))
            if not alive.size:
                continue
            rays = ray_index[:, y0:y1, x0:x1].reshape(-1)
            U = (_lines(o[rays], d[rays]) @ edges.reshape(T, 3, 6)[alive].reshape(-1, 6).T).reshape(-1, alive.size, 3) * keep_sign
            r, t = np.nonzero((U >= 0).all(axis=2) & (U.sum(axis=2) > 0))
            u = U[r, t]
            hr.append(rays[r]), ht.append(alive[t]), hb.append(u / u.sum(axis=1, keepdims=True))
    if not hr:
        hr, ht, hb = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [np.zeros((0, 3))]
    hr, ht, hb = np.concatenate(hr), np.concatenate(ht), np.concatenate(hb)

    point = np.einsum("nk,nkc->nc", hb, P[ht])
    clip = np.concatenate([point, np.ones((point.shape[0], 1))], axis=1) @ VP
    with np.errstate(all="ignore"):
        z = clip[:, 2] / clip[:, 3]
    ok = ((z >= 0) & (z <= 1)) if light else ((clip[:, 3] > 0) & (clip[:, 2] <= clip[:, 3]))
    return {"w": w, "h": h, "light": light, "V": V, "VP": VP, "along": along, "o": o, "d": d, "P": P, "N": N, "C": C, "UV": UV, "TAN": TAN, "owner": owner,
            "local": local, "base": np.stack(base) if base else np.zeros((0, 3)), "ray": hr[ok], "tri": ht[ok], "bary": hb[ok], "point": point[ok], "z": z[ok]}


def winners(H, chosen):
    """cast()'s dict from hits() and the indices of the hit each ray keeps (at most one per ray)."""
    w, h, light, V, VP, along, o, d, P, N, C, owner, local = (H[k] for k in ("w", "h", "light", "V", "VP", "along", "o", "d", "P", "N", "C", "owner", "local"))
    hr, ht, hb, point, z = (H[k][chosen] for k in ("ray", "tri", "bary", "point", "z"))
    R = o.shape[0]
    out = {"hit": np.zeros(R, bool), "draw": np.full(R, -1), "tri": np.full(R, -1), "gtri": np.full(R, -1), "depth": np.full(R, np.nan),
           "view_depth": np.full(R, np.nan), "normal": np.full((R, 3), np.nan), "albedo": np.full((R, 3), np.nan), "index": np.full(R, -1)}
    out["index"][hr] = chosen  # (the kept hit's place in hits()' arrays)
    out["hit"][hr], out["draw"][hr], out["tri"][hr], out["gtri"][hr], out["depth"][hr] = True, owner[ht], local[ht], ht, z
    out["view_depth"][hr] = -(point @ along[:3] + along[3])
    with np.errstate(all="ignore"):
        n = np.einsum("nk,nkc->nc", hb, N[ht])
        n = n / np.linalg.norm(n, axis=1, keepdims=True)
        m = n @ (np.eye(3) if light else V[:3, :3])
        out["normal"][hr] = m / np.linalg.norm(m, axis=1, keepdims=True)
    out["albedo"][hr] = H["base"][owner[ht]] * np.einsum("nk,nkc->nc", hb, C[ht][:, :, :3])
    out = {k: v.reshape((9, h, w) + v.shape[1:]) for k, v in out.items()}

    # the sheet test's prediction: the view depths at which the 9 rays meet the plane of the centre ray's triangle
    g = np.maximum(out["gtri"][0].reshape(-1), 0)
    a0, nrm = P[g, 0], np.cross(P[g, 1] - P[g, 0], P[g, 2] - P[g, 0])
    o9, d9 = o.reshape(9, h * w, 3), d.reshape(9, h * w, 3)
    with np.errstate(all="ignore"):
        t = np.einsum("rc,krc->kr", nrm, a0[None] - o9) / np.einsum("rc,krc->kr", nrm, d9)
        plane_vd = -((o9 + t[..., None] * d9) @ along[:3] + along[3])
    out["plane_spread"] = (plane_vd.max(axis=0) - plane_vd.min(axis=0)).reshape(h, w)
    out["altitude"] = _altitudes(P, VP, w, h, light)
    return out


def _altitudes(P, VP, w, h, light):
    """The smallest altitude, in px, of each triangle as the target sees it. A triangle that crosses w = z (the near plane) is first cut
    there - the part in front is a triangle or a quadrilateral - and a quadrilateral counts as the thinnest of the four triangles its two
    diagonals make, so nothing here depends on how the rule splits it. Triangles wholly behind get infinity: no ray hits them."""
    out = np.full(P.shape[0], np.inf)
    for k in range(P.shape[0]):
        c = np.concatenate([P[k], np.ones((3, 1))], axis=1) @ VP
        inside = np.ones(3, bool) if light else (c[:, 3] - c[:, 2] >= 0)
        poly = []
        for i in range(3):
            j = (i + 1) % 3
            if inside[i]:
                poly.append(c[i])
            if inside[i] != inside[j]:
                di, dj = c[i, 3] - c[i, 2], c[j, 3] - c[j, 2]
                poly.append(c[i] + di / (di - dj) * (c[j] - c[i]))
        if len(poly) < 3:
            continue
        q = np.array(poly)
        s = np.stack([(q[:, 0] / q[:, 3] + 1.0) * 0.5 * w, (1.0 - q[:, 1] / q[:, 3]) * 0.5 * h], axis=1)
        for a, b, e in ([(0, 1, 2)] if len(poly) == 3 else [(0, 1, 2), (0, 2, 3), (1, 2, 3), (0, 1, 3)]):
            area2 = abs((s[b, 0] - s[a, 0]) * (s[e, 1] - s[a, 1]) - (s[e, 0] - s[a, 0]) * (s[b, 1] - s[a, 1]))
            longest = max(np.hypot(*(s[b] - s[a])), np.hypot(*(s[e] - s[b])), np.hypot(*(s[a] - s[e])))
            out[k] = min(out[k], area2 / longest if longest > 0 else 0.0)
    return out


# ---- which texels are compared, and how closely ----------------------------------------------------------------------------------------

def classify(rc):
    """(compared (h, w) bool, hit_any (h, w) bool, left-out share of the texels any ray hits)."""
    hit = rc["hit"]
    all_hit, none_hit = hit.all(axis=0), ~hit.any(axis=0)
    one_draw = (rc["draw"] == rc["draw"][0]).all(axis=0)
    alt = np.where(hit, rc["altitude"][np.maximum(rc["gtri"], 0)], np.inf).min(axis=0)
    with np.errstate(all="ignore"):
        vd = rc["view_depth"]
        spread = np.where(all_hit, vd.max(axis=0) - vd.min(axis=0), 0.0)
        one_sheet = spread <= SHEET_FACTOR * rc["plane_spread"] + _ROUNDING * np.abs(vd[0])
    compared = none_hit | (all_hit & one_draw & (alt >= MIN_ALTITUDE_PX) & one_sheet)
    any_hit = hit.any(axis=0)
    return compared, any_hit, float((any_hit & ~compared).sum()) / max(int(any_hit.sum()), 1)


def _spread(v):
    with np.errstate(all="ignore"):
        return np.max(v, axis=0) - np.min(v, axis=0)


def _fraction(err, tol, mask):
    """(number of masked values with err > tol, largest err / tol over the mask)."""
    if not mask.any():
        return 0, 0.0
    e, t = err[mask], tol[mask]
    bad = ~(e <= t)  # (a NaN fails)
    return int(bad.sum()), float(np.max(np.where(np.isfinite(e), e, np.inf) / t))


def compare_depth(rc, target, bound: float, clear: float):
    """A depth target against the cast: {"covered": (failures, 0 or inf), "depth": (failures, largest error / tolerance)}."""
    compared, _, _ = classify(rc)
    t = np.asarray(target, np.float64)
    hit = rc["hit"][0] & compared
    miss = ~rc["hit"][0] & compared
    wrong = (miss & (t != clear)) | (hit & (t == clear))
    fails, worst = _fraction(np.abs(t - rc["depth"][0]), _spread(rc["depth"]) + bound, hit & ~wrong)
    return {"covered": (int(wrong.sum()), np.inf if wrong.any() else 0.0), "depth": (fails, worst)}


def fp16_ulp(x):
    """The spacing of fp16 at |x| (of the subnormals below 2^-14)."""
    return np.exp2(np.floor(np.log2(np.maximum(np.abs(x), 2.0 ** -14))) - 10)


def srgb8(x):
    """The sRGB code of a linear value: the standard curve, rounded to nearest, in float64."""
    x = np.clip(np.asarray(x, np.float64), 0.0, 1.0)
    return np.floor(255.0 * np.where(x <= 0.0031308, 12.92 * x, 1.055 * x ** (1.0 / 2.4) - 0.055) + 0.5).astype(np.int64)


CLEAR_HALF = np.array([0, 0, 0, 0x3C00], np.uint16)


def compare_gbuffer(rc, out, draws, a_ulps: float, c_codes: int):
    """A gbuffer result (the dict of gbuffer_ref.gbuffer_pass or gbuffer_gpu.run) against the cast: {output: (failures, largest error /
    tolerance)}; the exact outputs report 0 or inf."""
    compared, _, _ = classify(rc)
    hit, miss = rc["hit"][0] & compared, ~rc["hit"][0] & compared
    who = np.maximum(rc["draw"][0], 0)
    half = lambda v: np.asarray(v, np.float32).astype(np.float16).view(np.uint16)  # noqa: E731
    want_b = np.stack([np.concatenate([half([0.04, d.metallic, d.roughness]), CLEAR_HALF[3:]]) for d in draws])[who]
    want_hdr = np.stack([np.concatenate([half(d.emissive), CLEAR_HALF[3:]]) for d in draws])[who]
    want_id = np.array([d.object_id for d in draws], np.uint32)[who]
    want_b[~rc["hit"][0]], want_hdr[~rc["hit"][0]], want_id[~rc["hit"][0]] = CLEAR_HALF, CLEAR_HALF, 0
    res = {}

    def exact(name, bad):
        bad = bad & compared
        res[name] = (int(bad.sum()), np.inf if bad.any() else 0.0)

    exact("B", (out["B"] != want_b).any(axis=-1))
    exact("hdr", (out["hdr"] != want_hdr).any(axis=-1))
    if "object_id" in out:
        exact("object_id", out["object_id"] != want_id)
    exact("covered", (miss & ((out["A"] != CLEAR_HALF).any(axis=-1) | (out["C"] != 0xFF000000))) |
          (hit & (out["B"][..., 0] == 0)))  # (B.x is fp16 0.04 wherever a draw was resolved)

    with np.errstate(all="ignore"):
        a = out["A"].view(np.float16).astype(np.float64)
        ref = np.concatenate([rc["normal"], rc["view_depth"][..., None]], axis=-1)  # (9, h, w, 4)
        fails, worst = _fraction(np.abs(a - ref[0]), _spread(ref) + a_ulps * fp16_ulp(ref[0]), hit[..., None] & np.ones(4, bool))
        res["A"] = (fails, worst)
        code = np.stack([(out["C"] >> s) & 0xFF for s in (0, 8, 16)], axis=-1).astype(np.int64)
        lo, hi = srgb8(np.min(rc["albedo"], axis=0)), srgb8(np.max(rc["albedo"], axis=0))
        fails, worst = _fraction(np.abs(code - srgb8(rc["albedo"][0])).astype(np.float64), (hi - lo + c_codes).astype(np.float64),
                                 hit[..., None] & np.ones(3, bool))
        alpha = hit & ((out["C"] >> 24) != 0xFF)
        res["C"] = (fails + int(alpha.sum()), np.inf if alpha.any() else worst)
    return res


def failures(res) -> int:
    return sum(v[0] for v in res.values())


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------

@dataclass
class Scene:
    name: str
    draws: list
    view: "np.ndarray | None" = None
    proj: "np.ndarray | None" = None
    lvp: "np.ndarray | None" = None


NEAR = 0.125
FOV_Y = np.pi / 4


def _camera(eye, direction, w, h):
    from unclerenderer_amd import hostmath
    return hostmath.look_to_lh(eye, direction), hostmath.reverse_z_projection(FOV_Y, w / h, NEAR)


def _rotation(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def _world(rotation, scale, translation):
    """rotation x scale x translation for row vectors: v' = ((v R) S) + t."""
    W = np.eye(4)
    W[:3, :3] = rotation @ np.diag(scale)
    W[3, :3] = translation
    return W.astype(np.float32).reshape(-1)


def _outward_front(pos, faces, outward):
    """Wind every face so that the side `outward` points to is the front: seen from there the geometric normal (v1 - v0) x (v2 - v0)
    must point away from the viewer, that is against `outward` (see the module docstring)."""
    f = np.array(faces, np.int64)
    n = np.cross(pos[f[:, 1]] - pos[f[:, 0]], pos[f[:, 2]] - pos[f[:, 0]])
    flip = (n * outward[f].mean(axis=1)).sum(axis=1) > 0
    f[flip] = f[flip][:, [0, 2, 1]]
    return f


def icosphere_mesh(subdivisions: int = 2):
    """(positions (162, 3), faces (320, 3)) for two subdivisions of the icosahedron, vertices shared, outside = front."""
    g = (1.0 + np.sqrt(5.0)) / 2.0
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdivisions):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    pos = np.array(v)
    return pos, _outward_front(pos, f, pos)


def torus_mesh(major: int = 16, minor: int = 12, R: float = 1.0, r: float = 0.55):
    """(positions, normals, faces): major x minor segments, vertices shared, outside = front."""
    u, t = np.meshgrid(np.arange(major) * 2 * np.pi / major, np.arange(minor) * 2 * np.pi / minor, indexing="ij")
    nrm = np.stack([np.cos(u) * np.cos(t), np.sin(t), np.sin(u) * np.cos(t)], axis=-1).reshape(-1, 3)
    pos = np.stack([R * np.cos(u), np.zeros_like(u), R * np.sin(u)], axis=-1).reshape(-1, 3) + r * nrm
    f = []
    for i in range(major):
        for j in range(minor):
            a, b = i * minor + j, ((i + 1) % major) * minor + j
            c, e = i * minor + (j + 1) % minor, ((i + 1) % major) * minor + (j + 1) % minor
            f += [(a, b, e), (a, e, c)]
    return pos, nrm, _outward_front(pos, f, nrm)


def _gdraw(pos, nrm, col, faces, world, **kw):
    return GDraw(vertex_buffer(pos, nrm, col), np.asarray(faces, np.uint32).reshape(-1), world, **kw)


def icosphere_draw(seed: int = 1, translation=(0.3, -0.2, 3.2)):
    rng = np.random.default_rng(seed)
    pos, faces = icosphere_mesh()
    world = _world(_rotation((1, 2, 3), 0.7), (1.3, 0.8, 1.0), translation)
    return _gdraw(pos, pos, rng.uniform(0.1, 1.0, pos.shape), faces, world, base_color=np.array([0.9, 0.7, 0.5], np.float32),
                  emissive=np.array([0.5, 0.0, 2.0], np.float32), metallic=0.25, roughness=0.5, object_id=7)


def torus_draw(seed: int = 2, translation=(-0.2, 0.1, 3.4)):
    rng = np.random.default_rng(seed)
    pos, nrm, faces = torus_mesh()
    world = _world(_rotation((3, 1, -2), 1.1), (1.2, 1.2, 0.9), translation)
    return _gdraw(pos, nrm, rng.uniform(0.1, 1.0, pos.shape), faces, world, base_color=np.array([0.4, 0.8, 1.0], np.float32),
                  emissive=np.array([0.0, 1.5, 0.25], np.float32), metallic=0.75, roughness=0.125, object_id=0x80000021)


CAMERA_EYE, CAMERA_DIR = (0.4, 0.3, -0.5), (-0.12, -0.08, 1.0)


def icosphere_scene(w, h):
    view, proj = _camera(CAMERA_EYE, CAMERA_DIR, w, h)
    return Scene("icosphere", [icosphere_draw()], view, proj)


def torus_scene(w, h):
    view, proj = _camera(CAMERA_EYE, CAMERA_DIR, w, h)
    return Scene("torus", [torus_draw()], view, proj)


def two_draws_scene(w, h):
    """Icosphere and torus through each other. The cast does not know an order of draws; the passes run it in both."""
    view, proj = _camera(CAMERA_EYE, CAMERA_DIR, w, h)
    return Scene("two draws", [icosphere_draw(translation=(0.1, 0.0, 3.3)), torus_draw()], view, proj)


def strip_scene(w, h):
    """An 8 x 2 grid of quads from behind the camera to the distance - it passes the near plane inside the view, below the eye - and, under
    it, two triangles larger than the target that cross the near plane too. Colour and normal vary along the strip."""
    eye, direction = (0.0, 0.0, 0.0), (0.05, 0.03, 1.0)
    view, proj = _camera(eye, direction, w, h)
    a, b, across = np.array([-0.05, -0.1, -1.5]), np.array([1.5, 1.0, 22.0]), np.array([0.28, 0.03, 0.0])
    s = np.linspace(0.0, 1.0, 9) ** 2  # short quads by the camera, long ones in the distance
    pos = np.array([a + si * (b - a) + (j - 1) * across for si in s for j in range(3)])
    nrm = np.array([[0.6 * np.sin(5 * si) + 0.2 * (j - 1), 1.0, 0.5 * np.cos(3 * si)] for si in s for j in range(3)])
    col = np.array([[0.1 + 0.9 * si, 0.9 - 0.8 * si, 0.3 + 0.3 * j] for si in s for j in range(3)])
    faces = []
    for i in range(8):
        for j in range(2):
            v = i * 3 + j
            faces += [(v, v + 3, v + 4), (v, v + 4, v + 1)]
    toward_eye = np.asarray(eye) - pos
    strip = _gdraw(pos, nrm, col, _outward_front(pos, faces, toward_eye), _world(np.eye(3), (1, 1, 1), (0, 0, 0)),
                   base_color=np.array([1.0, 0.8, 0.6], np.float32), emissive=np.array([0.25, 0.5, 0.0], np.float32), metallic=0.5,
                   roughness=0.75, object_id=3)
    fpos = np.array([[-40.0, -1.5, -5.0], [40.0, -1.4, -5.0], [40.0, -1.2, 60.0], [-40.0, -1.6, 60.0]])
    fnrm = np.array([[0.1, 1.0, 0.0], [-0.2, 1.0, 0.1], [0.0, 1.0, -0.3], [0.3, 1.0, 0.2]])
    fcol = np.array([[1.0, 0.2, 0.2], [0.2, 1.0, 0.2], [0.2, 0.2, 1.0], [1.0, 1.0, 0.2]])
    floor = _gdraw(fpos, fnrm, fcol, _outward_front(fpos, [(0, 1, 2), (0, 2, 3)], np.asarray(eye) - fpos),
                   _world(np.eye(3), (1, 1, 1), (0, 0, 0)), base_color=np.array([0.5, 0.5, 0.9], np.float32),
                   emissive=np.array([0.0, 0.0, 1.0], np.float32), metallic=0.0, roughness=1.0, object_id=4)
    return Scene("near-plane strip", [strip, floor], view, proj)


def shadow_scene(w, h):
    """Icosphere + torus under the light's orthographic view of their bounding sphere; the target's size does not enter the matrix."""
    from unclerenderer_amd import hostmath
    draws = [icosphere_draw(translation=(0.1, 0.0, 3.3)), torus_draw()]
    pts = np.concatenate([_mesh(d)[0].reshape(-1, 3) @ _m4(d.world)[:3, :3] + _m4(d.world)[3, :3] for d in draws])
    centre = 0.5 * (pts.min(axis=0) + pts.max(axis=0))
    radius = float(np.linalg.norm(pts - centre, axis=1).max())
    return Scene("shadow", draws, lvp=hostmath.light_view_projection(centre, radius, (-0.3, 0.8, -0.5)))


CAMERA_SCENES = {"icosphere": icosphere_scene, "torus": torus_scene, "near-plane strip": strip_scene, "two draws": two_draws_scene}

_CASTS = {}


def cast_scene(name: str, w: int, h: int):
    """(scene, cast), cached per scene and target: the cast does not depend on the order of the draws."""
    if (name, w, h) not in _CASTS:
        sc = shadow_scene(w, h) if name == "shadow" else CAMERA_SCENES[name](w, h)
        _CASTS[(name, w, h)] = (sc, cast(sc.draws, w, h, sc.view, sc.proj, sc.lvp))
    return _CASTS[(name, w, h)]
