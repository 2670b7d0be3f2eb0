"""The environment from a panorama (csrc/env_panorama_rule.h) restated in numpy, and what its tests share.

build(rgbe, W, H, E, K, dt) is the rule: dt = np.float32 follows csrc/env_panorama_rule.h operation by operation - the integer-built
texel value, the written-out atan2, the 64-lane summing order - and gives the host build's bytes; dt = np.float64 is the same rule with
numpy's arctan2 and no rounding between steps, the yardstick of the fp32 arithmetic. Both return the taps' panorama texels too, so that
a comparison can leave out the output texels where the two precisions take other taps. `fault` plants one error (FAULTS).
The tests' own .hdr writer (hdr_file: flat and run-length coded), an RGBE encoder, an analytic environment with its float64 quadrature
over a cube texel - an independent definition: no panorama, no taps, no atan2 polynomial - and exact solid angles are here as well."""
import numpy as np

FAULTS = ("u_mirrored", "v_flipped", "seam_clamped", "mantissa_plus_half", "exponent_128", "no_clamp", "point_sampled", "no_plus_one")
F32 = np.float32


# ---- files
def rle_plane(values):
    """One channel of a scanline as new-style RLE: runs of three and more as (128 + n, value), the rest as (n, n literals)."""
    out, i, n = bytearray(), 0, len(values)
    literals = bytearray()

    def flush():
        nonlocal literals
        while literals:
            out.append(min(len(literals), 128))
            out.extend(literals[:128])
            literals = literals[128:]
    while i < n:
        j = i
        while j < n and values[j] == values[i] and j - i < 127:
            j += 1
        if j - i >= 3:
            flush()
            out.extend((128 + (j - i), values[i]))
        else:
            literals.extend(values[i:j])
        i = j
    flush()
    return bytes(out)


def hdr_file(rgbe, rle, magic=b"#?RADIANCE", lines=(b"# written by the tests", b"FORMAT=32-bit_rle_rgbe", b"EXPOSURE=1.0"), resolution=None):
    """rgbe uint8 [H, W, 4] as a .hdr file's bytes; rle: run-length coded scanlines (the width must be 8..32767) or the flat payload."""
    h, w = rgbe.shape[:2]
    head = b"\n".join((magic,) + tuple(lines)) + b"\n\n" + (resolution if resolution is not None else b"-Y %d +X %d" % (h, w)) + b"\n"
    if not rle:
        return head + np.ascontiguousarray(rgbe, np.uint8).tobytes()
    body = bytearray()
    for y in range(h):
        body.extend((2, 2, w >> 8, w & 255))
        for c in range(4):
            body.extend(rle_plane(bytes(rgbe[y, :, c])))
    return head + bytes(body)


def to_rgbe(rgb):
    """float64 [..., 3] >= 0 to the nearest RGBE bytes under the decode m * 2^(e - 136): the largest channel's mantissa in 128..255."""
    rgb = np.asarray(rgb, np.float64)
    top = rgb.max(axis=-1)
    _, ex = np.frexp(np.where(top > 0, top, 1.0))
    m = np.rint(rgb * np.ldexp(1.0, 8 - ex)[..., None])
    over = m.max(axis=-1) > 255
    ex = ex + over
    m = np.where(over[..., None], np.rint(rgb * np.ldexp(1.0, 8 - ex)[..., None]), m)
    e = ex + 128
    ok = (top > 0) & (e >= 1) & (e <= 255)
    out = np.zeros(rgb.shape[:-1] + (4,), np.uint8)
    out[..., :3] = np.where(ok[..., None], m, 0)
    out[..., 3] = np.where(ok, e, 0)
    return out


def random_panorama(seed, w, h):
    """Seeded RGBE texels [h, w, 4]: every mantissa, exponents mostly around 1.0 with some far below (subnormal values, e = 0) and above
    (beyond fp16), and runs along the rows so that the RLE writer has both kinds of packet."""
    rng = np.random.default_rng(seed)
    out = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    e = rng.integers(118, 140, (h, w))
    wild = rng.random((h, w))
    e = np.where(wild < 0.05, rng.integers(0, 12, (h, w)), e)
    e = np.where(wild > 0.97, rng.integers(140, 256, (h, w)), e)
    out[..., 3] = e
    if w >= 8:
        out[:, w // 2:w // 2 + 5] = out[:, w // 2:w // 2 + 1]
    return out


# ---- the rule
def rgbe_values(rgbe, dt=F32, fault=None):
    """[..., 4] uint8 to [..., 3] values: m * 2^(e - 136), 0 when e == 0; exact in either precision."""
    m, e = rgbe[..., :3].astype(np.float64), rgbe[..., 3].astype(np.int64)
    if fault == "mantissa_plus_half":
        m = m + 0.5
    v = np.ldexp(m, (e - (128 if fault == "exponent_128" else 136))[..., None])
    return np.where((e == 0)[..., None], 0.0, v).astype(dt)


ATAN_P = (F32(0.07882428169250488), F32(-0.13817109167575836), F32(0.19971036911010742), F32(-0.3333272635936737), F32(1.0))


def atan2_rule(y, x):
    """csrc/env_panorama_rule.h's atan2_rule on float32 arrays, operation by operation."""
    y, x = np.broadcast_arrays(np.asarray(y, F32), np.asarray(x, F32))
    ax, ay = np.abs(x), np.abs(y)
    hi, lo = np.where(ax > ay, ax, ay), np.where(ax > ay, ay, ax)
    zero = ~(hi > 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        a = lo / np.where(zero, F32(1), hi)
    upper = a > F32(0.41421357)
    r = np.where(upper, (a - F32(1)) / (a + F32(1)), a)
    s = r * r
    p = ATAN_P[0]
    for c in ATAN_P[1:]:
        p = p * s + c
    angle = r * p
    angle = np.where(upper, F32(0.78539816339744831) + angle, angle)
    angle = np.where(ay > ax, F32(1.57079632679489662) - angle, angle)
    angle = np.where(x < 0, F32(3.14159265358979324) - angle, angle)
    return np.where(zero, F32(0), np.copysign(angle, y)).astype(F32)


def face_direction(face, s, t):
    one = np.ones_like(s)
    return [(one, -t, -s), (-one, -t, s), (s, one, t), (s, -one, -t), (s, -t, one), (-s, -t, -one)][face]


def taps_of(w, h, base):
    k = 1
    while k < 16 and (3 * k * base < 2 * w or 3 * k * base < 4 * h):
        k *= 2
    return k


def tap_samples(rgbe, w, h, base, taps, dt=F32, fault=None):
    """Every tap of every output texel: (values [6, E, E, K * K, 3] in dt, the taps' first panorama texel [6, E, E, K * K, 2] as (row, column)
    before wrap and clamp). Tap index i = sy * K + sx."""
    E, K = base, taps
    values = rgbe_values(np.asarray(rgbe, np.uint8).reshape(h, w, 4), dt, fault)
    n = np.arange(E * K, dtype=np.uint32)
    plus = 0 if fault == "no_plus_one" else 1
    c = ((2 * n + plus).astype(dt) / dt(K * E) - dt(1)).astype(dt)
    if fault == "point_sampled":  # K ignored: every tap at the texel's centre
        centre = ((2 * (n // K) + 1).astype(dt) / dt(E) - dt(1)).astype(dt)
        c = centre
    # [E, K] per axis -> [E(y), E(x), K(sy), K(sx)]
    cs = c.reshape(E, K)
    s = np.broadcast_to(cs[None, :, None, :], (E, E, K, K)).reshape(E, E, K * K)
    t = np.broadcast_to(cs[:, None, :, None], (E, E, K, K)).reshape(E, E, K * K)
    out, where = np.zeros((6, E, E, K * K, 3), dt), np.zeros((6, E, E, K * K, 2), np.int64)
    for face in range(6):
        dx, dy, dz = (np.asarray(a, dt) for a in face_direction(face, s, t))
        if dt == F32:
            az = atan2_rule(dx, dz)
            el = atan2_rule(dy, np.sqrt(dx * dx + dz * dz))
            u = F32(0.5) + az * F32(0.15915494309189535)
            v = F32(0.5) - el * F32(0.31830988618379069)
        else:
            az = np.arctan2(dx, dz)
            az = np.where((dx == 0) & (dz == 0), 0.0, az)
            u = 0.5 + az / (2 * np.pi)
            v = 0.5 - np.arctan2(dy, np.sqrt(dx * dx + dz * dz)) / np.pi
        if fault == "u_mirrored":
            u = dt(1) - u
        if fault == "v_flipped":
            v = dt(1) - v
        px, py = u * dt(w) - dt(0.5), v * dt(h) - dt(0.5)
        x0, y0 = np.floor(px), np.floor(py)
        fx, fy = (px - x0)[..., None], (py - y0)[..., None]
        ix, iy = x0.astype(np.int64), y0.astype(np.int64)
        if fault == "seam_clamped":
            c0, c1 = np.clip(ix, 0, w - 1), np.clip(ix + 1, 0, w - 1)
        else:
            c0, c1 = ix % w, (ix + 1) % w
        r0, r1 = np.clip(iy, 0, h - 1), np.clip(iy + 1, 0, h - 1)
        a, b, c_, d = values[r0, c0], values[r0, c1], values[r1, c0], values[r1, c1]
        with np.errstate(over="ignore", invalid="ignore"):  # (only a planted error gets there)
            top, bottom = a + fx * (b - a), c_ + fx * (d - c_)
            out[face] = top + fy * (bottom - top)
        where[face, ..., 0], where[face, ..., 1] = iy, ix
    return out, where


def lane_sum(tap_values):
    """[..., K * K, 3] -> [..., 3] in the rule's order: lane j of 64 from +0 adds taps j, j + 64, ... ascending; a tree by strides 32 .. 1."""
    dt = tap_values.dtype
    n = tap_values.shape[-2]
    lanes = np.zeros(tap_values.shape[:-2] + (64, 3), dt)
    for first in range(0, n, 64):
        chunk = tap_values[..., first:first + 64, :]
        lanes[..., :chunk.shape[-2], :] = lanes[..., :chunk.shape[-2], :] + chunk
    stride = 32
    while stride:
        lanes = lanes[..., :stride, :] + lanes[..., stride:2 * stride, :]
        stride //= 2
    return lanes[..., 0, :]


def build(rgbe, w, h, base, taps, dt=F32, fault=None):
    """The rule. dt = float32: (the cube's top level as uint16 [6, E, E, 4], the taps' texels). dt = float64: (the means before the
    clamp and the rounding as float64 [6, E, E, 3], the taps' texels)."""
    values, where = tap_samples(rgbe, w, h, base, taps, dt, fault)
    with np.errstate(over="ignore"):
        mean = lane_sum(values) * dt(1.0 / (taps * taps))
    if dt != F32:
        return mean, where
    if fault != "no_clamp":
        mean = np.where(mean < F32(65504), mean, F32(65504))
    out = np.zeros((6, base, base, 4), np.uint16)
    with np.errstate(over="ignore"):
        out[..., :3] = mean.astype(np.float16).view(np.uint16)
    out[..., 3] = 0x3C00
    return out, where


def half_ulps(got_bits, want):
    """The distance of fp16 bit patterns `got_bits` (finite, >= 0) from float64 values `want` in units of the fp16 spacing at `want`."""
    got = got_bits.view(np.float16).astype(np.float64)
    w = np.minimum(np.abs(want), 65504.0)
    ulp = np.ldexp(1.0, np.maximum(np.floor(np.log2(np.maximum(w, 2.0 ** -14))), -14).astype(np.int64) - 10)
    return np.abs(got - np.minimum(want, 65504.0)) / ulp


# ---- the independent definition: an analytic environment
def environment(seed):
    """radiance(d [..., 3] unit) -> [..., 3]: 1 + a direction-linear gradient + two broad lobes, channels within a factor of two of each
    other; and its mean over the sphere is about 1."""
    rng = np.random.default_rng(seed)
    grad = rng.normal(size=3)
    grad *= 0.3 / np.linalg.norm(grad)
    axes = rng.normal(size=(2, 3))
    axes /= np.linalg.norm(axes, axis=1, keepdims=True)
    tint = 0.75 + 0.5 * rng.random((3, 3))  # per term and channel, in [0.75, 1.25]

    def radiance(d):
        d = np.asarray(d, np.float64)
        base = 1.0 + d @ grad
        lobes = [np.maximum(d @ axes[k], 0.0) ** (4 + 4 * k) for k in range(2)]
        return base[..., None] * tint[0] + lobes[0][..., None] * tint[1] + 0.5 * lobes[1][..., None] * tint[2]
    return radiance


def panorama_directions(w, h):
    """The unit directions of the panorama's texel centres [h, w, 3]: u = (x + 0.5) / w around +Y from -Z through +X, v = (y + 0.5) / h."""
    az = ((np.arange(w) + 0.5) / w - 0.5) * 2 * np.pi
    el = (0.5 - (np.arange(h) + 0.5) / h) * np.pi
    ce = np.cos(el)[:, None]
    return np.stack([ce * np.sin(az)[None, :], np.broadcast_to(np.sin(el)[:, None], (h, w)), ce * np.cos(az)[None, :]], axis=-1)


def quadrature(radiance, base, n=16):
    """The expected cube [6, E, E, 3]: per texel the float64 n x n midpoint mean of the analytic function over the texel's square in (s, t)."""
    c = (2 * np.arange(base * n) + 1) / (base * n) - 1
    s, t = np.meshgrid(c, c)
    out = np.zeros((6, base, base, 3))
    for face in range(6):
        d = np.stack(face_direction(face, s, t), axis=-1)
        d = d / np.linalg.norm(d, axis=-1, keepdims=True)
        out[face] = radiance(d).reshape(base, n, base, n, 3).mean(axis=(1, 3))
    return out


# ---- solid angles
def corner_area(x, y):
    return np.arctan2(x * y, np.sqrt(x * x + y * y + 1.0))


def cube_texel_solid_angles(base):
    """[E, E]: the exact solid angle of every texel of a face (the same for all six); they add up to 4 pi / 6."""
    e = 2 * np.arange(base + 1) / base - 1
    a = corner_area(e[None, :], e[:, None])
    return a[1:, 1:] - a[1:, :-1] - a[:-1, 1:] + a[:-1, :-1]


def panorama_rows_solid_angle(h, w, y0, y1, columns):
    """The exact solid angle of `columns` panorama columns over rows y0 .. y1 - 1."""
    return (2 * np.pi * columns / w) * (np.sin((0.5 - y0 / h) * np.pi) - np.sin((0.5 - y1 / h) * np.pi))
