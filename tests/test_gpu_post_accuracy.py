"""The post chain's kernels against the float64 restatement (tests/post_ref64.py) at the sizes they run at: Tonemap and CAS under
the decided-byte rule, TemporalAA bit-exact against the oracle and under the fp16 rule, AutoExposure within tau_ae. Above
1080p the float64 side runs on samples (about 2e5 random pixels plus full rows and columns); whole frames are compared with
the oracle."""
import math

import numpy as np
import pytest

from tests import post_ref64 as P

pytestmark = pytest.mark.gpu

SPECIAL = [(float("inf"), 0, 0), (float("inf"),) * 3, (float("nan"), 0, 0), (0, float("nan"), 0.5), (float("-inf"), 0.5, 0.5),
           (-1.0, 0.5, 0.5), (65504.0, 0, 0), (65504.0,) * 3, (-0.0, -0.0, -0.0), (2.0 ** -24, 2.0 ** -20, 6.1e-5), (-65504.0, 0, 0),
           (0.08, 0.5, 0.9), (0.76, 0.76, 0.76), (1e-4, 1e-5, 0)]
TM_PARAMS = [dict(), dict(enable_tonemap=False), dict(exposure=0.9, gamma=2.2), dict(exposure=2.0, exposure_ev=-1.5)]


def _torch():
    import torch
    return torch


def _frame(h, w, seed):
    """rng ** 3 * 6 HDR (test_tonemap_parity's), with the SPECIAL pixels at even and odd positions of the first row and of a
    middle row."""
    rng = np.random.default_rng(seed)
    hdr = np.empty((h, w, 4), np.float16)
    hdr[..., :3] = (rng.random((h, w, 3), np.float32) ** 3 * 6.0).astype(np.float16)
    hdr[..., 3] = 2.0
    n = min(len(SPECIAL), w)
    for r in {0, h // 2}:
        hdr[r, :n, :3] = SPECIAL[:n]
        if w >= 2 * n + 1:
            hdr[r, n + 1:2 * n + 1, :3] = SPECIAL[:n]
    return hdr.view(np.uint16)


def _sample(h, w, seed, n=200_000):
    """(ys, xs): random pixels plus full first / middle / last rows and columns."""
    if h * w <= n:
        ys, xs = np.mgrid[0:h, 0:w]
        return ys.ravel(), xs.ravel()
    rng = np.random.default_rng(seed)
    ys, xs = [rng.integers(0, h, n)], [rng.integers(0, w, n)]
    for r in (0, h // 2, h - 1):
        ys.append(np.full(w, r)); xs.append(np.arange(w))
    for c in (0, w // 2 + 1, w - 1):
        ys.append(np.arange(h)); xs.append(np.full(h, c))
    return np.concatenate(ys), np.concatenate(xs)


def _non_finite(bits):
    return ~np.isfinite(P.hdr64(bits)[..., :3]).all(-1)


def _tonemap_rule(got_u32, bits, ys, xs, kw, what, record_property=None):
    """The decided-byte rule on the sampled pixels; pixels with a NaN or Inf channel byte-equal to the oracle instead."""
    sb = bits[ys, xs]
    lin, v, comp = P.tonemap64(sb, **kw)
    dec, want = P.tonemap_decide(lin, comp, kw.get("gamma", 2.2))
    got = P.channels(got_u32[ys, xs])
    fin = ~_non_finite(sb)
    r = P.byte_check(got[fin], dec[fin], want[fin], P.tonemap_bytes(v[fin]))
    if record_property:
        record_property(f"{what} wrong", r["wrong"])
        record_property(f"{what} undecided", r["undecided"])
        record_property(f"{what} misround", r["misround"])
    assert r["wrong"] == 0, (what, r)
    assert r["undecided"] <= P.UNDECIDED_MAX, (what, r)
    return r


def _old_rule(got, ref, what):
    d = np.abs(P.channels(got) - P.channels(ref))
    assert d.max() <= 1 and (d > 0).mean() < 2e-3, (what, int(d.max()), float((d > 0).mean()))


def _special_exact(got, ref, bits, what):
    nf = _non_finite(bits)
    assert np.array_equal(got[nf], ref[nf]), (what, np.flatnonzero(got[nf] != ref[nf])[:8])


@pytest.mark.parametrize("h,w", [(64, 257), (1080, 1920), (2160, 3840), (4320, 7680)])
def test_tonemap_decided_bytes(hotpath, oracle, h, w, record_property):
    """Every parameter set of test_tonemap_parity plus an EV from ur_auto_exposure; 8K runs the kPairTrips = 2 form (>= 24 M
    pixels). Whole frames are also held to the old tolerance and the non-finite pixels to the oracle's bytes."""
    torch = _torch()
    from unclerenderer_amd.hotpath import to_device
    bits = _frame(h, w, h + w)
    d = to_device(bits)
    ys, xs = _sample(h, w, 1)
    ev_t = torch.zeros(1, device="cuda")
    hotpath.auto_exposure(d, ev_t, w, h)
    torch.cuda.synchronize()
    ae_ev = float(ev_t.cpu()[0])
    params = TM_PARAMS + [dict(exposure=0.9, exposure_ev=ae_ev)]
    if h * w > 1920 * 1080:
        params = [TM_PARAMS[0], TM_PARAMS[3], params[-1]]
    out = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    for kw in params:
        ev = torch.tensor([kw["exposure_ev"]], device="cuda") if "exposure_ev" in kw else None
        out.fill_(0)
        hotpath.tonemap(d, out, w, h, exposure=kw.get("exposure", 1.0), gamma=kw.get("gamma", 2.2), enable_tonemap=kw.get("enable_tonemap", True),
                        exposure_ev=ev)
        torch.cuda.synchronize()
        got = out.cpu().numpy().view(np.uint32)
        _tonemap_rule(got, bits, ys, xs, kw, f"{kw}", record_property)
        ref = oracle.tonemap(bits, **kw)
        _old_rule(got, ref, kw)
        _special_exact(got, ref, bits, kw)


def test_tonemap_launch_forms_decided_bytes(hotpath, oracle, record_property):
    """1080p through the one-pixel form (HDR only 8-byte aligned), an odd pixel count (pairs + the last pixel) and row bands:
    each under the rule and byte-equal to the whole-frame launch."""
    torch = _torch()
    from unclerenderer_amd.hotpath import to_device
    h, w = 1080, 1920
    bits = _frame(h, w, 77)
    d = to_device(bits)
    kw = dict(exposure=0.9, gamma=2.2)
    full = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    hotpath.tonemap(d, full, w, h, **kw)
    flat_in, n = d.reshape(-1, 4), h * w
    # the one-pixel form: pixels 1 .. n-1 (HDR 8-byte aligned, odd count)
    one = torch.zeros(n, dtype=torch.int32, device="cuda")
    hotpath.tonemap(flat_in[1:], one[1:], n - 1, 1, **kw)
    # pairs + the odd last pixel: pixels 0 .. n-2
    odd = torch.zeros(n, dtype=torch.int32, device="cuda")
    hotpath.tonemap(flat_in[:n - 1], odd[:n - 1], n - 1, 1, **kw)
    # row bands: uneven cuts
    bands = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    for r0, r1 in ((0, 1), (1, 333), (333, 334), (334, h)):
        hotpath.tonemap(d[r0:r1], bands[r0:r1], w, r1 - r0, **kw)
    torch.cuda.synchronize()
    f = full.reshape(-1)
    assert torch.equal(one[1:], f[1:]) and torch.equal(odd[:n - 1], f[:n - 1]) and torch.equal(bands, full)
    got = full.cpu().numpy().view(np.uint32)
    ys, xs = _sample(h, w, 2, n=h * w)
    _tonemap_rule(got, bits, ys, xs, kw, "forms", record_property)
    _special_exact(got, oracle.tonemap(bits, **kw), bits, "forms")


def test_non_finite_and_edge_pixels_through_both_launches(hotpath, oracle):
    """The SPECIAL pixels through ur_tonemap and ur_tonemap_cas (sharpness 0: CAS returns its input bytes): NaN / Inf pixels
    byte-equal to the oracle, the rest under the rule."""
    torch = _torch()
    from unclerenderer_amd.hotpath import to_device
    h, w = 9, 67
    bits = _frame(h, w, 5)
    d = to_device(bits)
    ys, xs = _sample(h, w, 0)
    for kw in TM_PARAMS:
        ev = torch.tensor([kw["exposure_ev"]], device="cuda") if "exposure_ev" in kw else None
        a = torch.zeros((h, w), dtype=torch.int32, device="cuda")
        b = torch.zeros((h, w), dtype=torch.int32, device="cuda")
        tk = dict(exposure=kw.get("exposure", 1.0), gamma=kw.get("gamma", 2.2), enable_tonemap=kw.get("enable_tonemap", True), exposure_ev=ev)
        hotpath.tonemap(d, a, w, h, **tk)
        hotpath.tonemap_cas(d, b, w, h, sharpness=0.0, **tk)
        torch.cuda.synchronize()
        ref = oracle.tonemap(bits, **kw)
        for got in (a.cpu().numpy().view(np.uint32), b.cpu().numpy().view(np.uint32)):
            _special_exact(got, ref, bits, kw)
            _tonemap_rule(got, bits, ys, xs, kw, f"special {kw}")


def _cas_rule(got_u32, ldr_u32, s, rows, what, record_property=None):
    """CAS's decided-byte rule on whole rows `rows` (sorted, unique), the exact value computed from ldr_u32 (the kernel's own
    tonemap bytes for the fused launch)."""
    h, w = ldr_u32.shape
    wrong, n, und = 0, 0, 0.0
    for r in rows:
        lo = max(int(r) - 1, 0)  # rows r - 1 .. r + 1: the slice's edges are the image's where they clamp
        x = P.cas64(ldr_u32[lo:int(r) + 2], s, int(r) - lo, 1)
        dec, want = P.cas_decide(x)
        r_ = P.byte_check(P.channels(got_u32[r:r + 1]), dec, want)
        wrong += r_["wrong"]
        und += r_["undecided"] * r_["n"]
        n += r_["n"]
    if record_property:
        record_property(f"{what} wrong", wrong)
        record_property(f"{what} undecided", und / n)
    assert wrong == 0, (what, wrong)
    assert und / n <= P.UNDECIDED_MAX, (what, und / n)


def _cas_rows(h, k=24, seed=0):
    rng = np.random.default_rng(seed)
    return np.unique(np.concatenate([[0, 1, 7, 8, h // 2, h - 2, h - 1], rng.integers(0, h, k)]))


@pytest.mark.parametrize("h,w", [(2160, 3840), (4320, 7680)])
def test_cas_and_fused_decided_bytes(hotpath, h, w, record_property):
    """ur_cas of the tonemapped frame and ur_tonemap_cas, sharpness 0.5 and 1.0, on whole rows (strip edges included), plus a
    band of the fused launch whose rows start off the 8-row strip grid."""
    torch = _torch()
    from unclerenderer_amd.hotpath import to_device
    bits = _frame(h, w, 3 * h)
    d = to_device(bits)
    ldr = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    hotpath.tonemap(d, ldr, w, h, exposure=0.9, gamma=2.2)
    torch.cuda.synchronize()
    ldr_np = ldr.cpu().numpy().view(np.uint32)
    rows = _cas_rows(h)
    out = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    for s in (0.5, 1.0):
        hotpath.cas(ldr, out, w, h, sharpness=s)
        torch.cuda.synchronize()
        _cas_rule(out.cpu().numpy().view(np.uint32), ldr_np, s, rows, f"cas s={s}", record_property)
        hotpath.tonemap_cas(d, out, w, h, exposure=0.9, gamma=2.2, sharpness=s)
        torch.cuda.synchronize()
        _cas_rule(out.cpu().numpy().view(np.uint32), ldr_np, s, rows, f"fused s={s}", record_property)
    r0, n = h // 3 + 3, 13
    band = torch.zeros((n, w), dtype=torch.int32, device="cuda")
    hotpath.tonemap_cas(d, band, w, h, row0=r0, rows=n, exposure=0.9, gamma=2.2, sharpness=1.0)
    torch.cuda.synchronize()
    full = np.zeros((h, w), np.uint32)
    full[r0:r0 + n] = band.cpu().numpy().view(np.uint32)
    _cas_rule(full, ldr_np, 1.0, np.arange(r0, r0 + n), "fused band")


# ---- TemporalAA --------------------------------------------------------------------------------------------------------------
def _taa_frames(h, w, seed):
    rng = np.random.default_rng(seed)
    cur = (rng.random((h, w, 4), np.float32) ** 2 * 8).astype(np.float16)
    hist = (rng.random((h, w, 4), np.float32) ** 2 * 8).astype(np.float16)
    cur[..., 3] = 2.0
    return cur.view(np.uint16), hist.view(np.uint16)


@pytest.mark.parametrize("h,w", [(2160, 3840), (4320, 7680), (2251, 4001)])
def test_temporal_aa_large_frames(hotpath, oracle, h, w, record_property):
    """Whole frames bit-exact against the oracle with and without history; bands whose row0 is off the 8-row grid (a 1-row
    band, one ending at the last row); the fp16 rule (R1 with the cancellation allowance, R3) on a sample."""
    torch = _torch()
    from unclerenderer_amd.hotpath import to_device
    cb, hb = _taa_frames(h, w, h + w)
    d_cur, d_hist = to_device(cb), to_device(hb)
    out = torch.zeros((h, w, 4), dtype=torch.int16, device="cuda")
    for use, wt in ((True, 0.9), (False, 0.9)):
        hotpath.temporal_aa(d_cur, d_hist, out, wt, use, w, h)
        torch.cuda.synchronize()
        got = out.cpu().numpy().view(np.uint16)
        assert np.array_equal(got, oracle.temporal_aa(cb, hb, wt, use)), use
    # history on: `got` holds the last use=False run; redo with history for the rule and the bands
    hotpath.temporal_aa(d_cur, d_hist, out, 0.9, True, w, h)
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint16)
    ys, xs = _sample(h, w, 4)
    x, bound = P.temporal_aa64(cb, hb, 0.9, pixels=(ys, xs), with_bound=True)
    m = P.measure(got[ys, xs], x, np.zeros(len(ys), bool))
    record_property("max_e", float(np.nanmax(np.abs(m["e"]))))
    record_property("mean_e", m["mean"])
    record_property("misround", m["misround"])
    assert not P.r1_violations(m["e"], bound).any() and m["nan_mismatch"] == 0
    assert abs(m["mean"]) <= 0.02
    for r0, n in ((13, 1), (5, 22), (h - 7, 7), (h // 2 + 3, 40)):
        band = torch.zeros((n, w, 4), dtype=torch.int16, device="cuda")
        hotpath.temporal_aa(d_cur, d_hist[r0:r0 + n], band, 0.9, True, w, h, r0, n)
        torch.cuda.synchronize()
        assert np.array_equal(band.cpu().numpy().view(np.uint16), got[r0:r0 + n]), (r0, n)


TAA_SPECIAL = [0x7E00, 0x7D00, 0xFD00, 0x7E01, 0x0000, 0x8000, 0x0001, 0x8001, 0x03FF, 0x7C00, 0xFC00]


def test_temporal_aa_special_values_in_every_position(hotpath, oracle):
    """Quiet NaN, signalling-NaN patterns, +-0, subnormals and +-Inf in the centre, in the columns left of lane 0 and right of
    lane 63 of a wave, in the halo rows of an 8-row strip, at the frame edges and in the history: bit-exact against the oracle,
    whose min / max ignore every NaN as HLSL's do (NaN results: NaN in both, see below). Each value takes each position in
    its own channel pattern."""
    torch = _torch()
    from unclerenderer_amd.hotpath import to_device
    h, w = 26, 200
    cur, hist = _taa_frames(h, w, 3)
    cols = [0, 1, 62, 63, 64, 65, 126, 127, 128, 129, 191, 199]
    rows = [0, 1, 6, 7, 8, 9, 15, 16, 24, 25]
    k = 0
    for y in rows:
        for x in cols:
            v = TAA_SPECIAL[k % len(TAA_SPECIAL)]
            ch = k % 3
            cur[y, x, ch] = v
            if k % 4 == 0:
                cur[y, x, :3] = v
            if k % 5 == 0:
                hist[(y + 3) % h, (x + 7) % w, ch] = TAA_SPECIAL[(k + 3) % len(TAA_SPECIAL)]
            k += 1
    # the case that once failed: a signalling NaN right of lane 63 (halo column, v_readlane) and -Inf in lane 62 of one row -
    # v_pk_min_f16(-Inf, sNaN) is NaN, which dropped the -Inf from the box of lane 63 in the row above
    cur[20, 64, :3] = 0x7D00
    cur[20, 62, 2] = 0xFC00
    cur[19, 63, 2] = np.float16(6.5).view(np.uint16)
    hist[19, 63, 2] = np.float16(0.25).view(np.uint16)
    d_cur, d_hist = to_device(cur), to_device(hist)
    out = torch.zeros((h, w, 4), dtype=torch.int16, device="cuda")
    for wt in (0.9, 0.35, 1.0, 0.0):
        hotpath.temporal_aa(d_cur, d_hist, out, wt, True, w, h)
        torch.cuda.synchronize()
        got, ref = out.cpu().numpy().view(np.uint16), oracle.temporal_aa(cur, hist, wt, True)
        # a NaN result is a NaN in both, but its sign and payload are the hardware's: x86 returns the first NaN operand of
        # c + w * (h - c), the GPU's subtract flips the sign of a NaN c (and Inf - Inf gives opposite default NaNs). HLSL does
        # not define them, and Tonemap saturates any NaN to 0. Every other value is bit-exact.
        nan_g, nan_r = np.isnan(got.view(np.float16)), np.isnan(ref.view(np.float16))
        assert np.array_equal(nan_g, nan_r), wt
        bad = np.argwhere((got != ref) & ~nan_r)
        assert len(bad) == 0, (wt, [(tuple(b), hex(got[tuple(b)]), hex(ref[tuple(b)])) for b in bad[:6]])
        # and the oracle's finite values are the restatement's, rounded once (the kernel's min / max semantics are HLSL's)
        x, bound = P.temporal_aa64(cur, hist, wt, with_bound=True)
        m = P.measure(ref, x, np.zeros((h, w), bool))
        assert m["nan_mismatch"] == 0 and not P.r1_violations(m["e"], bound).any(), wt


# ---- AutoExposure ------------------------------------------------------------------------------------------------------------
def _ev(hotpath, d_hdr, w, h, **kw):
    torch = _torch()
    out = torch.full((1,), float("nan"), device="cuda")
    hotpath.auto_exposure(d_hdr, out, w, h, **kw)
    torch.cuda.synchronize()
    return float(out.cpu()[0])


def _hdr_bits(h, w, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    base = 0.05 + 2.0 * (x / max(w - 1, 1)) * (y / max(h - 1, 1))
    hdr = np.zeros((h, w, 4), np.float16)
    hdr[..., :3] = np.minimum(base[..., None] * (rng.random((h, w, 3)) ** 2 * 3.0) * scale, 60000).astype(np.float16)
    hdr[..., 3] = 1.0
    return hdr.view(np.uint16)


@pytest.mark.parametrize("h,w", [(1080, 1920), (2160, 3840), (131, 257), (9, 17), (1, 1), (1, 37), (37, 1), (15, 15), (16, 16), (17, 16)])
def test_auto_exposure_within_tau(hotpath, h, w, record_property):
    torch = _torch()
    from unclerenderer_amd.hotpath import to_device
    bits = _hdr_bits(h, w, 11)
    d = to_device(bits)
    exact, tau = P.auto_exposure64(bits), P.ae_tau(bits)
    got = _ev(hotpath, d, w, h)
    record_property("err", got - exact)
    record_property("tau", tau)
    assert abs(got - exact) <= tau, (got, exact, tau)
    for prev in (exact - 1.5, exact + 1.5):  # the history step, both speed directions
        kw = dict(use_history=True, delta_time=1 / 30, speed_up=3.0, speed_down=1.0)
        got = _ev(hotpath, d, w, h, prev_ev=torch.tensor([float(prev)], dtype=torch.float32, device="cuda"), **kw)
        want, t = P.auto_exposure64(bits, prev=prev, **kw), P.ae_tau(bits, prev=prev, **kw)
        record_property(f"prev {prev - exact:+} err", got - want)
        assert abs(got - want) <= t, (prev, got, want, t)


def test_auto_exposure_non_finite_frames(hotpath):
    from unclerenderer_amd.hotpath import to_device
    min_ev = math.log2(float(np.float32(0.1)))
    # an Inf texel on the last corner of tap (0, 0) of a 32 x 32 frame (weights 0.5, 0.5): log2(Inf) -> the target clamps to minEv
    bits = _hdr_bits(32, 32, 2)
    bits[1, 1, :3] = 0x7C00
    exact = P.auto_exposure64(bits)
    assert exact == min_ev
    assert abs(_ev(hotpath, to_device(bits), 32, 32) - exact) <= P.ae_tau(bits)
    # all NaN: luminance floored at 1e-4 (a high maxEv so that the clamp does not hide it)
    nan = np.full((24, 40, 4), 0x7E00, np.uint16)
    kw = dict(ev_max=1e6)
    exact = P.auto_exposure64(nan, **kw)
    assert math.isclose(exact, math.log2(float(np.float32(0.3))) - math.log2(float(np.float32(1e-4))), rel_tol=1e-15)
    assert abs(_ev(hotpath, to_device(nan), 40, 24, **kw) - exact) <= P.ae_tau(nan, **kw)
