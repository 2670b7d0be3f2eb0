"""The BRDF LUT (csrc/brdf_lut_rule.h) restated in numpy: the rule in fp32, operation by operation, whose bytes
ur_host_brdf_lut must give; the same rule in float64 with its own sample table; an independent float64 Gauss-Legendre integration of the
same BRDF over the half vector's hemisphere; and the planted errors."""
import numpy as np

from tests.env_sky_ref import lane_sum

F = np.float32


def hammersley(S):
    """(xi1, xi2) of section 3.20's point set, float64 [S]: i / S and the radical inverse of i in base 2."""
    i = np.arange(S, dtype=np.uint64)
    b = np.zeros(S, np.uint64)
    for bit in range(32):
        b |= ((i >> np.uint64(bit)) & np.uint64(1)) << np.uint64(31 - bit)
    return i.astype(np.float64) / S, b.astype(np.float64) / 4294967296.0


def table64(H, S):
    """The GGX importance half vectors in float64 [H, S, 3] for alpha = ((y + 0.5) / H)^2."""
    xi1, xi2 = hammersley(S)
    r = (np.arange(H, dtype=np.float64) + 0.5) / H
    a2 = ((r * r) ** 2)[:, None]
    cos2 = (1.0 - xi2) / (1.0 + (a2 - 1.0) * xi2)
    sine, phi = np.sqrt(1.0 - cos2), 2.0 * np.pi * xi1
    return np.stack([sine * np.cos(phi), sine * np.sin(phi), np.sqrt(cos2)], -1)


def sample_terms(nov, vx, alpha, hx, hz, T, nol_test=True):
    """One sample's (scale, bias) terms in the rule's order, arrays broadcast together; 0 where NoL <= 0."""
    voh = vx * hx + nov * hz
    nol = (T(2) * voh) * hz - nov
    oma = T(1) - alpha
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        vis = T(0.5) / (nol * (nov * oma + alpha) + nov * (nol * oma + alpha))
        w = (nol * vis) * ((T(4) * voh) / hz)
        m = T(1) - voh
        m2 = m * m
        fc = (m2 * m2) * m
        scale, bias = (T(1) - fc) * w, fc * w
    if nol_test:
        keep = nol > T(0)
        scale, bias = np.where(keep, scale, T(0)), np.where(keep, bias, T(0))
    return scale, bias


def unorm16(mean):
    """clamp to [0, 1] (a NaN gives 0), times 65535, to nearest even -> uint16."""
    v = np.where(mean > 0, np.minimum(mean, mean.dtype.type(1)), mean.dtype.type(0)) * mean.dtype.type(65535)
    return np.rint(v).astype(np.uint16)


def lut32(table, W, H, S, swap=False, alpha_is_roughness=False, nol_test=True):
    """The rule in fp32 over the table's bytes (uint8 or float32, [H, S, 4]) -> uint16 [H, W, 2]: the bytes of ur_host_brdf_lut."""
    tab = np.ascontiguousarray(table).view(F).reshape(-1, S, 4)
    x = (np.arange(W, dtype=F) + F(0.5)) / F(W)
    y = (np.arange(H, dtype=F) + F(0.5)) / F(H)
    nov, r = (y[:, None], x[None, :]) if swap else (x[None, :], y[:, None])
    nov, r = np.broadcast_to(nov, (H, W)), np.broadcast_to(r, (H, W))
    alpha = r if alpha_is_roughness else r * r
    vx = np.sqrt(F(1) - nov * nov)
    rows = tab[None, :W] if swap else tab[:H, None]  # [H or 1, 1 or W, S, 4]
    hx, hz = rows[..., 0], rows[..., 2]
    scale, bias = sample_terms(nov[..., None], vx[..., None], alpha[..., None].astype(F), hx, hz, F, nol_test)
    with np.errstate(invalid="ignore", over="ignore"):
        sums = lane_sum(np.stack([scale, bias], -1).astype(F))
        return unorm16(sums * F(1.0 / S))


def lut64(W, H, S):
    """The rule in float64 with its own table -> float64 [H, W, 2] in [0, 1], unrounded (the plain mean: float64 needs no order)."""
    tab = table64(H, S)
    nov = np.broadcast_to(((np.arange(W) + 0.5) / W)[None, :, None], (H, W, 1))
    r = ((np.arange(H) + 0.5) / H)[:, None, None]
    scale, bias = sample_terms(nov, np.sqrt(1.0 - nov * nov), r * r, tab[:, None, :, 0], tab[:, None, :, 2], np.float64)
    return np.clip(np.stack([scale.mean(-1), bias.mean(-1)], -1), 0.0, 1.0)


def quadrature(W, H, nodes=48, phi_nodes=128):
    """(scale, bias) by Gauss-Legendre panels over the half vector's polar angle - breakpoints at multiples of atan(alpha), where the GGX
    lobe lives - and its azimuth (half of it: the integrand is even in phi), in float64 [H, W, 2]. The integral is
    int D(h) (n.h) Vis (n.l) 4 (v.h) / (n.h) [1 - Fc, Fc] dh over the h with n.l > 0: no sample is shared with the rule, and neither is the
    parametrisation (no importance transform)."""
    gx, gw = np.polynomial.legendre.leggauss(nodes)
    px, pw = np.polynomial.legendre.leggauss(phi_nodes)
    phi, wphi = (px + 1.0) * (np.pi / 2.0), pw * (np.pi / 2.0) * 2.0  # [0, pi], doubled
    out = np.zeros((H, W, 2))
    for y in range(H):
        r = (y + 0.5) / H
        alpha = r * r
        a2 = alpha * alpha
        lobe = np.arctan(alpha)
        breaks = [0.0] + [lobe * f for f in (0.25, 0.5, 1, 2, 4, 8, 16, 32, 64, 128, 256, 1024) if lobe * f < np.pi / 2] + [np.pi / 2]
        th = np.concatenate([(gx + 1) * 0.5 * (b - a) + a for a, b in zip(breaks[:-1], breaks[1:])])
        wth = np.concatenate([gw * 0.5 * (b - a) for a, b in zip(breaks[:-1], breaks[1:])])
        ch, sh = np.cos(th), np.sin(th)
        t = ch * ch * (a2 - 1.0) + 1.0
        D = a2 / (np.pi * t * t)
        hx, hz = (sh[:, None] * np.cos(phi)[None, :]), np.broadcast_to(ch[:, None], (len(th), len(phi)))
        weight = (D * ch * sh * wth)[:, None] * wphi[None, :]  # D (n.h) sin(theta) dtheta dphi
        for x in range(W):
            nov = (x + 0.5) / W
            scale, bias = sample_terms(nov, np.sqrt(1.0 - nov * nov), alpha, hx, hz, np.float64)
            out[y, x] = (scale * weight).sum(), (bias * weight).sum()
    return out
