"""A numpy restatement of the environment prefilter (include/ur_env_prefilter.h), written from DESIGN.md section 3.20, not from the C++:

  table      Hammersley points, GGX half vectors, the mirrored light vector and the source level, in float64, rounded to fp32
  pyramid    2 x 2 box means, ((t00 + t10) + (t01 + t11)) * 0.25, a level rounded once to fp16
  borders    the fold of tests/env_cube_ref.py (the restatement of the staging rule, section 3.19)
  filter     per output texel the centre's direction, Duff's frame, per kept sample one trilinear sample of the bordered pyramid; lane j
             of 64 adds the samples j, j + 64, ... ascending, the lanes meet in a tree by strides 32 .. 1, one multiply by the level's
             reciprocal weight, one rounding to fp16

prefilter() runs it in a chosen precision: np.float32 is the rule to the byte, np.float64 the same rule with the sampling and the sums in
float64 (the table stays the fp32 table). It also returns every sample's taps (face, column, row, lower level) so that a comparison can
leave out the texels where the two precisions take other taps. `fault` plants one error (FAULTS). quadrature() is the independent
definition: it shares no step with any of this."""
import numpy as np

from tests import env_cube_ref as CUBE

FAULTS = ("alpha_r", "neg_y_tc", "no_weight", "lod0", "prev_table", "unnormalised", "clamped")
LANES = 64


def levels_of(base):
    return base.bit_length()


def radical_inverse(i):
    return int(format(i, "032b")[::-1], 2) / 4294967296.0


def table(base, samples, fault=None, bias=0.0):
    """[(inv_weight fp32, kept, entries fp32 [S, 4])] for the levels 0 .. L - 1 (level 0: (1, 0, None)); a dropped sample is a zero row.
    bias: the constant added to the source level (the rule's is 0; others are for the measurement DESIGN.md 3.20 records)."""
    L = levels_of(base)
    out = [(np.float32(1.0), 0, None)]
    omega_p = 4.0 * np.pi / (6.0 * base * base)
    i = np.arange(samples)
    xi1 = i / samples
    xi2 = np.array([radical_inverse(int(v)) for v in i])
    for k in range(1, L):
        r = k / (L - 1)
        alpha = r if fault == "alpha_r" else r * r
        a2 = alpha * alpha
        cos2 = (1.0 - xi2) / (1.0 + (a2 - 1.0) * xi2)
        hz, sine = np.sqrt(cos2), np.sqrt(1.0 - cos2)
        phi = 2.0 * np.pi * xi1
        hx, hy = sine * np.cos(phi), sine * np.sin(phi)
        t = cos2 * (a2 - 1.0) + 1.0
        D = a2 / (np.pi * t * t)
        lod = np.clip(0.5 * np.log2((4.0 / (samples * D)) / omega_p) + bias, 0.0, L - 1.0)
        e = np.stack([2.0 * hz * hx, 2.0 * hz * hy, 2.0 * cos2 - 1.0, lod], axis=1).astype(np.float32)
        kept = e[:, 2] > 0
        e[~kept] = 0
        out.append((np.float32(1.0 / e[kept, 2].astype(np.float64).sum()), int(kept.sum()), e))
    return out


def table_from_bytes(raw, base, samples):
    """ur_host_env_prefilter_table's bytes in table()'s form."""
    L = levels_of(base)
    raw = np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
    head = raw[:16 * L]
    out = []
    for k in range(L):
        inv, kept = head[16 * k:16 * k + 4].view(np.float32)[0], int(head[16 * k + 4:16 * k + 8].view(np.uint32)[0])
        e = raw[16 * L + 16 * samples * (k - 1):16 * L + 16 * samples * k].view(np.float32).reshape(samples, 4) if k else None
        out.append((inv, kept, e))
    return out


def pyramid(top):
    """top uint16 [6, E, E, 4] -> [float16 [6, n, n, 3]] for every level."""
    level = np.ascontiguousarray(top).view(np.float16)[..., :3]
    out = [level]
    while level.shape[1] > 1:
        v = level.astype(np.float32)
        level = (((v[:, 0::2, 0::2] + v[:, 0::2, 1::2]) + (v[:, 1::2, 0::2] + v[:, 1::2, 1::2])) * np.float32(0.25)).astype(np.float16)
        out.append(level)
    return out


def bordered(levels, fault=None):
    """One flat array of every level's bordered faces [texels, 3] float16 and the levels' first texels."""
    parts, starts, at = [], [], 0
    for level in levels:
        n = level.shape[1]
        e = n + 2
        faces = np.zeros((6, e, e, 3), np.float16)
        faces[:, 1:n + 1, 1:n + 1] = level
        for f in range(6):
            for j in range(-1, n + 1):
                for i in range(-1, n + 1):
                    if 0 <= i < n and 0 <= j < n:
                        continue
                    sf, si, sj = (f, min(max(i, 0), n - 1), min(max(j, 0), n - 1)) if fault == "clamped" else CUBE.fold(n, f, i, j)
                    faces[f, j + 1, i + 1] = level[sf, sj, si]
        parts.append(faces.reshape(-1, 3))
        starts.append(at)
        at += 6 * e * e
    return np.concatenate(parts), starts


def directions(n, dt, fault=None):
    """The normalised directions of a level's texel centres, face-major, row-major: [6 n n, 3]."""
    c = (2 * np.arange(n) + 1).astype(dt) / dt(n) - dt(1)
    s, t = np.meshgrid(c, c, indexing="xy")
    one = np.ones_like(s)
    faces = [(one, -t, -s), (-one, -t, s), (s, one, t), (s, -one, t if fault == "neg_y_tc" else -t), (s, -t, one), (-s, -t, -one)]
    d = np.stack([np.stack(f, axis=-1) for f in faces]).reshape(-1, 3)
    length = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    return d / length[:, None]


def frame(n):
    """Duff's branch-free orthonormal frame around unit vectors [T, 3]: (tangent, bitangent)."""
    one = n.dtype.type(1)
    sign = np.copysign(one, n[:, 2])
    a = -one / (sign + n[:, 2])
    b = (n[:, 0] * n[:, 1]) * a
    tangent = np.stack([one + sign * ((n[:, 0] * n[:, 0]) * a), sign * b, -(sign * n[:, 0])], axis=1)
    bitangent = np.stack([b, sign + (n[:, 1] * n[:, 1]) * a, -n[:, 1]], axis=1)
    return tangent, bitangent


def face_uv(d):
    """D3D cube addressing of directions [..., 3] (ties z > y > x): face, u, v."""
    dt = d.dtype.type
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    ax, ay, az = np.abs(x), np.abs(y), np.abs(z)
    zmaj = (az >= ax) & (az >= ay)
    ymaj = ~zmaj & (ay >= ax)
    comp = np.where(zmaj, z, np.where(ymaj, y, x))
    face = np.where(zmaj, 4, np.where(ymaj, 2, 0)) + (comp < 0)
    ma = np.abs(comp)
    sc = np.select([face == 0, face == 1, face == 5], [-z, z, -x], x)
    tc = np.select([face == 2, face == 3], [z, -z], -y)
    return face, (sc / ma + dt(1)) * dt(0.5), (tc / ma + dt(1)) * dt(0.5)


def bilinear(flat, start, n, face, u, v):
    """One 2 x 2 sample of the bordered level of edge n (arrays: start and n per sample); (rgb, column, row)."""
    dt = u.dtype.type
    x, y = u * n.astype(u.dtype) - dt(0.5), v * n.astype(u.dtype) - dt(0.5)
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = (x - x0)[..., None], (y - y0)[..., None]
    i0, j0 = np.clip(x0.astype(np.int64) + 1, 0, n), np.clip(y0.astype(np.int64) + 1, 0, n)
    e = n + 2
    at = start + (face * e + j0) * e + i0
    t00, t10, t01, t11 = (flat[at + o].astype(u.dtype) for o in (0, 1, e, e + 1))
    top, bottom = t00 + fx * (t10 - t00), t01 + fx * (t11 - t01)
    return top + fy * (bottom - top), i0, j0


def prefilter(top, base, samples, tab, dt=np.float32, fault=None):
    """(the chain as uint16 [texels, 4] in DDS order, {k: taps int [T, S, 4]}). tab: table() or table_from_bytes()."""
    L = levels_of(base)
    top = np.ascontiguousarray(top).view(np.uint16).reshape(6, base, base, 4)
    pyr = pyramid(top)
    flat, starts = bordered(pyr, fault)
    starts = np.array(starts)
    sizes = np.array([base >> m for m in range(L)])
    out = [[None] * L for _ in range(6)]
    first = top.copy()
    first[..., 3] = 0x3C00
    for f in range(6):
        out[f][0] = first[f].reshape(-1, 4)
    taps = {}
    for k in range(1, L):
        n = base >> k
        inv, kept_count, e = tab[k]
        if fault == "prev_table":
            inv, kept_count, e = tab[k - 1] if k > 1 else (np.float32(1), 1, np.array([[0, 0, 1, 0]] + [[0, 0, 0, 0]] * (samples - 1), np.float32))
        e = e.astype(dt)
        lx, ly, lz, lod = e[:, 0], e[:, 1], e[:, 2], e[:, 3]
        if fault == "lod0":
            lod = np.zeros_like(lod)
        kept = lz > 0
        N = directions(n, dt, fault)
        T, B = frame(N)
        d = (T[:, None, :] * lx[None, :, None] + B[:, None, :] * ly[None, :, None]) + N[:, None, :] * lz[None, :, None]  # [texels, S, 3]
        d[:, ~kept] = N[:, None, :]  # (a dropped sample adds nothing: any finite direction will do)
        face, u, v = face_uv(d)
        lv = np.clip(lod, dt(0), dt(L - 1))
        m0 = lv.astype(np.int64)
        m1 = np.minimum(m0 + 1, L - 1)
        fl = (lv - m0.astype(dt))[None, :, None]
        lo, i0, j0 = bilinear(flat, starts[m0][None, :], sizes[m0][None, :], face, u, v)
        hi, _, _ = bilinear(flat, starts[m1][None, :], sizes[m1][None, :], face, u, v)
        rgb = np.where(fl != 0, lo + fl * (hi - lo), lo)
        weight = np.ones_like(lz) if fault == "no_weight" else lz
        term = np.where(kept[None, :, None], weight[None, :, None] * rgb, dt(0))
        padded = max(samples, LANES)
        if padded != samples:
            term = np.concatenate([term, np.zeros((term.shape[0], padded - samples, 3), dt)], axis=1)
        rounds = term.reshape(term.shape[0], padded // LANES, LANES, 3)
        lanes = np.zeros((term.shape[0], LANES, 3), dt)
        for r in range(rounds.shape[1]):
            lanes = lanes + rounds[:, r]
        stride = LANES // 2
        while stride:
            lanes = lanes[:, :stride] + lanes[:, stride:2 * stride]
            stride //= 2
        total = lanes[:, 0]
        if fault == "no_weight":
            total = total * dt(1.0 / kept_count)
        elif fault != "unnormalised":
            total = total * dt(inv)
        with np.errstate(over="ignore"):
            texels = np.concatenate([total.astype(np.float16).view(np.uint16), np.full((total.shape[0], 1), 0x3C00, np.uint16)], axis=1)
        for f in range(6):
            out[f][k] = texels[f * n * n:(f + 1) * n * n]
        sig = np.stack([face, i0, j0, np.broadcast_to(m0[None, :], face.shape)], axis=-1)
        sig[:, ~kept] = 0
        taps[k] = sig
    return np.concatenate([out[f][k] for f in range(6) for k in range(L)]), taps


def level_of_payload(payload, base, k):
    """Level k of a DDS-order payload uint16 [texels, 4] as [6, n, n, 4]."""
    L = levels_of(base)
    per_face = sum((base >> m) ** 2 for m in range(L))
    start, n = sum((base >> m) ** 2 for m in range(k)), base >> k
    return np.ascontiguousarray(payload).view(np.uint16).reshape(6, per_face, 4)[:, start:start + n * n].reshape(6, n, n, 4)


def random_cube(seed, base, peak=60000.0):
    """A seeded finite cube: values spread over many binades up to `peak`, a tenth of them negative."""
    rng = np.random.default_rng(seed)
    v = peak * rng.random((6, base, base, 4)) ** 4 * np.where(rng.random((6, base, base, 4)) < 0.1, -1.0, 1.0)
    return v.astype(np.float16).view(np.uint16)


# ---- the independent definition
def smooth_environment(seed):
    """A direction-linear gradient plus two broad lobes: a function of unit directions [..., 3] -> radiance [..., 3], positive."""
    rng = np.random.default_rng(seed)
    g = rng.uniform(-0.4, 0.4, (3, 3))
    axes = rng.normal(size=(2, 3))
    axes /= np.linalg.norm(axes, axis=1, keepdims=True)
    colours = rng.uniform(0.5, 3.0, (2, 3))

    def radiance(w):
        out = 1.0 + w @ g
        for a, c in zip(axes, colours):
            out = out + c * np.exp(4.0 * (w @ a - 1.0))[..., None]
        return out
    return radiance


def texel_grid(n):
    """Centre directions (unnormalised), and exact solid angles, of every texel of a cube of edge n: [6, n, n, 3], [n, n]."""
    edges = 2.0 * np.arange(n + 1) / n - 1.0
    c = 0.5 * (edges[:-1] + edges[1:])
    s, t = np.meshgrid(c, c, indexing="xy")
    one = np.ones_like(s)
    points = np.stack([np.stack(CUBE.POINT[f](s, t, one), axis=-1) for f in range(6)])
    corner = lambda x, y: np.arctan2(x * y, np.sqrt(x * x + y * y + 1.0))  # noqa: E731
    x0, x1 = np.meshgrid(edges[:-1], edges[:-1], indexing="xy"), np.meshgrid(edges[1:], edges[1:], indexing="xy")
    omega = corner(x1[0], x1[1]) - corner(x0[0], x1[1]) - corner(x1[0], x0[1]) + corner(x0[0], x0[1])
    return points, omega


def supersampled(radiance, base, factor=4):
    """(the fine cube's radiance [6, fn, fn, 3], directions, solid angles; the test cube uint16 [6, base, base, 4] of its box means)."""
    points, omega = texel_grid(base * factor)
    w = points / np.linalg.norm(points, axis=-1, keepdims=True)
    fine = radiance(w)
    coarse = fine.reshape(6, base, factor, base, factor, 3).mean(axis=(2, 4))
    cube = np.concatenate([coarse, np.ones((6, base, base, 1))], axis=-1).astype(np.float16).view(np.uint16)
    return fine, w, omega, cube


def quadrature(fine, w, omega, base, k, texels):
    """Level k's texels (indices into the level, face-major) by the definition: sum L D(n.h) (n.w) dO / sum D(n.h) (n.w) dO over every
    texel of the fine cube, h = normalize(n + w), D plain GGX at alpha = (k / (L - 1))^2. float64 [len(texels), 3]."""
    L = levels_of(base)
    alpha = (k / (L - 1)) ** 2
    a2 = alpha * alpha
    n_points, _ = texel_grid(base >> k)
    normals = (n_points / np.linalg.norm(n_points, axis=-1, keepdims=True)).reshape(-1, 3)[texels]
    w, fine, omega = w.reshape(-1, 3), fine.reshape(-1, 3), np.broadcast_to(omega, (6,) + omega.shape).reshape(-1)
    out = np.zeros((len(texels), 3))
    for i, n in enumerate(normals):
        nw = w @ n
        h = w + n
        nh = (h @ n) / np.linalg.norm(h, axis=1)
        t = nh * nh * (a2 - 1.0) + 1.0
        weight = np.where(nw > 0, a2 / (np.pi * t * t) * nw * omega, 0.0)
        out[i] = (weight[:, None] * fine).sum(axis=0) / weight.sum()
    return out
