"""The sky capture (csrc/env_sky_rule.h) restated in numpy: the rule in fp32, operation by operation, whose bytes
ur_host_env_sky must give; the same rule in float64; the face table; and the planted errors. No library code is used but the folded
constants, which come from hostmath.env_sky_params (their own float64 restatement is fold64)."""
import numpy as np

F = np.float32
LANES = 64
# (s, t) -> the direction on a face: +X (1, -t, -s)  -X (-1, -t, s)  +Y (s, 1, t)  -Y (s, -1, -t)  +Z (s, -t, 1)  -Z (-s, -t, -1)
FACES = [lambda s, t, o: (o, -t, -s), lambda s, t, o: (-o, -t, s), lambda s, t, o: (s, o, t), lambda s, t, o: (s, -o, -t), lambda s, t, o: (s, -t, o),
         lambda s, t, o: (-s, -t, -o)]
ZENITH, HORIZON, RAYLEIGH = (0.05, 0.12, 0.22), (0.52, 0.68, 0.86), (0.650, 0.570, 0.475)


def sky_constants(light_dir, light_color=(1.0, 0.95, 0.9), camera_y=1.5):
    from unclerenderer_amd import lib
    sky = lib.SkyConstants()
    sky.CameraPosition[:] = [3.0, camera_y, -2.0]
    sky.LightDirection[:] = list(light_dir)
    sky.LightColor[:] = list(light_color)
    for i in (0, 5, 10, 15):  # the matrices are not read: anything will do
        sky.World[i] = sky.View[i] = sky.Projection[i] = 7.0
    return sky


def fold64(sky):
    """The folded constants in float64, unrounded: (sun[3], scatter[3], mie[3], attenuation)."""
    c = lambda v: np.float64(F(v))  # noqa: E731  (a shader literal)
    pi, g = c(3.14159265), c(0.76)
    L = np.array(list(sky.LightDirection), np.float64)
    sun = L / np.sqrt((L * L).sum())
    h = max(0.0, float(sky.CameraPosition[1]))
    scatter = np.array([c(v) for v in RAYLEIGH]) * np.exp(-h / 8000.0) * (3.0 / (16.0 * pi))
    mie = np.array(list(sky.LightColor), np.float64) * np.exp(-h / 1200.0) * (c(0.8) * ((1.0 - g * g) / (4.0 * pi)))
    att = min(max(np.exp(-max(0.0, 1.0 - sun[1]) * 2.0), 0.0), 1.0)
    return sun, scatter, mie, att


def directions(E, K, dtype=F, flip=None):
    """The normalised tap directions [6, E, E, K * K, 3] (tap i = sy K + sx) by the rule's grid and face table."""
    T = dtype
    n = np.arange(E * K, dtype=np.uint32)
    coord = (2 * n + 1).astype(T) / T(K * E) - T(1)  # [E K]
    coord = coord.reshape(E, K)
    s = np.broadcast_to(coord[None, :, None, :], (E, E, K, K)).reshape(E, E, K * K)  # x, sx
    t = np.broadcast_to(coord[:, None, :, None], (E, E, K, K)).reshape(E, E, K * K)  # y, sy
    one = np.ones_like(s)
    out = np.empty((6, E, E, K * K, 3), T)
    for f in range(6):
        d = FACES[f](s, t, one)
        if flip is not None and flip[0] == f:
            d = tuple(-v if i == flip[1] else v for i, v in enumerate(d))
        dx, dy, dz = (np.asarray(v, T) for v in d)
        length = np.sqrt((dx * dx + dy * dy) + dz * dz)
        out[f, ..., 0], out[f, ..., 1], out[f, ..., 2] = dx / length, dy / length, dz / length
    return out


def sky_value(params, d, dtype=F, g_sign=1.0, exponent=3, ):
    """ApplyAtmosphere over the folded constants for unit directions d[..., 3], in the rule's order -> [..., 3]."""
    T = dtype
    sun, scatter, mie, att = (np.asarray(v, T) for v in params)
    sat = lambda x: np.minimum(np.maximum(x, T(0)), T(1))  # noqa: E731
    h = T(1) - sat(d[..., 1] * T(0.5) + T(0.5))
    fall = sat((h * h) * h) if exponent == 3 else sat(h * h)
    cos = (d[..., 0] * sun[0] + d[..., 1] * sun[1]) + d[..., 2] * sun[2]
    ray = T(1) + cos * cos
    g = T(F(0.76)) * T(g_sign)
    mb = (T(1) + g * g) - (T(2) * g) * cos
    denom = mb * np.sqrt(mb)
    phase = T(1) / np.maximum(denom, T(F(1e-3)))
    out = np.empty(d.shape, T)
    for c in range(3):
        z, hz = T(F(ZENITH[c])), T(F(HORIZON[c]))
        out[..., c] = (z + fall * (hz - z)) + (scatter[c] * ray + mie[c] * phase) * att
    return out


def lane_sum(taps):
    """Section 3.20's order over the last-but-one axis of taps[..., n, C] (fp32): lane j adds taps j, j + 64, ... from +0, then the tree."""
    n = taps.shape[-2]
    pad = (-n) % LANES
    if pad:
        taps = np.concatenate([taps, np.zeros(taps.shape[:-2] + (pad, taps.shape[-1]), taps.dtype)], axis=-2)
    rounds = taps.reshape(taps.shape[:-2] + (-1, LANES, taps.shape[-1]))
    lanes = np.zeros(rounds.shape[:-3] + rounds.shape[-2:], taps.dtype)
    for r in range(rounds.shape[-3]):
        lanes = lanes + rounds[..., r, :, :]
    stride = LANES // 2
    while stride:
        lanes = lanes[..., :stride, :] + lanes[..., stride:2 * stride, :]
        stride //= 2
    return lanes[..., 0, :]


def to_half_bits(mean):
    """min(., 65504) and one rounding to fp16 -> uint16 bits."""
    return np.minimum(mean, F(65504.0)).astype(np.float16).view(np.uint16)


def capture32(params, E, K, **planted):
    """The rule in fp32 -> uint16 [6, E, E, 4]: the bytes of ur_host_env_sky."""
    flip = planted.pop("flip", None)
    with np.errstate(over="ignore", invalid="ignore"):
        taps = sky_value(params, directions(E, K, F, flip), F, **planted)
        mean = lane_sum(taps) * F(1.0 / (K * K))
        out = np.empty((6, E, E, 4), np.uint16)
        out[..., :3] = to_half_bits(np.where(mean < F(65504.0), mean, F(65504.0)))
    out[..., 3] = 0x3C00
    return out


def capture64(params64, E, K):
    """The rule in float64 with the unrounded constants -> float64 [6, E, E, 3] (the plain mean: float64 needs no order)."""
    taps = sky_value(params64, directions(E, K, np.float64), np.float64)
    return np.minimum(taps.mean(axis=-2), 65504.0)


def half_ulp(x):
    """One fp16 ulp at |x| (float64): 2^(floor(log2 |x|) - 10), at least the subnormal step 2^-24."""
    e = np.floor(np.log2(np.maximum(np.abs(x), 2.0 ** -14)))
    return 2.0 ** (e - 10)


def cube_of(bits):
    """uint16 [6, E, E, 4] -> float64 [6, E, E, 3]."""
    return np.ascontiguousarray(bits).view(np.float16).astype(np.float64)[..., :3]
