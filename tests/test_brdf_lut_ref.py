"""The BRDF LUT without a GPU: ur_host_brdf_lut - the functions the kernel runs - against hand-worked answers, byte for
byte against the numpy fp32 restatement of tests/brdf_lut_ref.py, against the same rule in float64, against an independent float64
quadrature, against the shipped PreintegratedGF.dds, its bounds, and the planted errors, which each change bytes."""
import math

import numpy as np
import pytest

from tests import brdf_lut_ref as R
from tests.test_bcn_abi import ROOT

SIZES = [(1, 1), (3, 2), (7, 5), (64, 8), (128, 32)]
SAMPLES = [16, 64, 1024]
# measured here (DESIGN.md 3.22 records them); every bound below is twice its figure
MEASURED_RULE64 = 0.5048 / 65535              # largest |host - float64 rule| over the sizes and sample counts above: the rounding to UNORM16
MEASURED_QUADRATURE = (0.00838, 0.00090)           # largest |host - quadrature| at 16 x 8 x 1024: scale, bias
MEASURED_SHIPPED_MEAN = (0.00522, 0.00031)       # mean |host - shipped file| at 128 x 32 x 1024 over x >= 8: scale, bias
MEASURED_SHIPPED_MAX = (0.03058, 0.00354)        # and the largest


@pytest.fixture(scope="module")
def host_luts(urlib):
    """{(W, H, S): the host build}: computed once, shared and left unchanged."""
    from unclerenderer_amd import hostmath
    out = {}
    for W, H in SIZES + [(16, 8), (8, 8)]:
        for S in SAMPLES:
            lut = hostmath.brdf_lut(W, H, S)
            assert lut.shape == (H, W, 2) and lut.dtype == np.uint16
            lut.setflags(write=False)
            out[(W, H, S)] = lut
    return out


def test_one_texel_by_hand(host_luts):
    """1 x 1, 16 samples: NoV = 0.5, roughness 0.5, alpha 0.25, V = (sqrt(0.75), 0, 0.5). The arithmetic below is the rule with Python's
    floats, sample by sample: sample 0 is H = N (xi2 = 0): VoH = 0.5, NoL = 2 * 0.5 - 0.5 = 0.5, Vis = 0.5 / (2 * 0.5 * (0.5 * 0.75 + 0.25)) = 0.8,
    w = 0.5 * 0.8 * 4 * 0.5 / 1 = 0.8, Fc = 0.5^5 = 0.03125: scale takes 0.775, bias 0.025. The sixteen give 0.747262 and 0.020075."""
    scale = bias = 0.0
    terms = []
    for i in range(16):
        xi1, xi2 = i / 16, int(f"{i:04b}"[::-1], 2) / 16
        a2 = 0.25 ** 2
        cos2 = (1 - xi2) / (1 + (a2 - 1) * xi2)
        hz, hx = math.sqrt(cos2), math.sqrt(1 - cos2) * math.cos(2 * math.pi * xi1)
        voh = math.sqrt(0.75) * hx + 0.5 * hz
        nol = 2 * voh * hz - 0.5
        if nol > 0:
            vis = 0.5 / (nol * (0.5 * 0.75 + 0.25) + 0.5 * (nol * 0.75 + 0.25))
            w = nol * vis * 4 * voh / hz
            fc = (1 - voh) ** 5
            scale, bias = scale + (1 - fc) * w, bias + fc * w
            terms.append(((1 - fc) * w, fc * w))
    assert terms[0] == (0.775, 0.025)
    assert abs(scale / 16 - 0.747262) < 1e-6 and abs(bias / 16 - 0.020075) < 1e-6
    assert list(host_luts[(1, 1, 16)][0, 0]) == [round(scale / 16 * 65535), round(bias / 16 * 65535)] == [48972, 1316]


def test_row_zero_of_a_tall_table(urlib):
    """Row 0 of 256 rows: alpha = (1 / 512)^2 = 3.8e-6, every half vector is the normal but for an angle of about alpha, so w tends to
    VoH / (NoV NoH) = 1 and the texel to (1 - (1 - NoV)^5, (1 - NoV)^5). The half vectors' largest angle, tan = alpha sqrt(xi / (1 - xi)) with
    xi = 63 / 64, is 3e-5 rad; against NoV >= 1 / 32 that moves VoH by 1e-3 of itself at most: within 0.001 here (1e-4 measured)."""
    from unclerenderer_amd import hostmath
    lut = hostmath.brdf_lut(16, 256, 64).astype(np.float64) / 65535
    nov = (np.arange(16) + 0.5) / 16
    assert (np.abs(lut[0, :, 0] - (1 - (1 - nov) ** 5)) < 0.001).all() and (np.abs(lut[0, :, 1] - (1 - nov) ** 5) < 0.001).all()


def test_host_bytes_are_the_numpy_restatement(host_luts):
    from unclerenderer_amd import hostmath
    for W, H in SIZES:
        for S in SAMPLES:
            want = R.lut32(hostmath.brdf_lut_table(H, S), W, H, S)
            same = host_luts[(W, H, S)] == want
            assert same.all(), f"{W} x {H}, {S} samples: {np.count_nonzero(~same)} values differ, first at {tuple(np.argwhere(~same)[0])}"


def test_the_table_is_the_float64_table(urlib):
    from unclerenderer_amd import hostmath
    for H, S in ((1, 16), (5, 64), (32, 1024), (256, 16)):
        tab = hostmath.brdf_lut_table(H, S).view(np.float32).reshape(H, S, 4)
        want = R.table64(H, S)
        assert (tab[..., 3] == 0).all()
        # (sin, cos and sqrt of another library's double may differ in its last bit: at most one fp32 ulp of a value near 1 here)
        assert (np.abs(tab[..., :3].astype(np.float64) - want) <= 2.0 ** -23).all()
    assert int(hostmath._lib.load().ur_brdf_lut_table_bytes(32, 1024)) == 16 * 32 * 1024


def test_the_rule_in_float64(host_luts):
    worst = 0.0
    for W, H in SIZES:
        for S in SAMPLES:
            worst = max(worst, float(np.abs(host_luts[(W, H, S)].astype(np.float64) / 65535 - R.lut64(W, H, S)).max()))
    print(f"largest error against the float64 rule: {worst * 65535:.4f} UNORM16 steps")
    assert worst <= 2 * MEASURED_RULE64


def test_independent_quadrature(host_luts):
    """16 x 8 at 1024 samples against the Gauss-Legendre integration: what is measured is the Monte-Carlo error of the rule's 1024 points."""
    want = R.quadrature(16, 8)
    err = np.abs(host_luts[(16, 8, 1024)].astype(np.float64) / 65535 - want).reshape(-1, 2).max(axis=0)
    print(f"largest error against the quadrature at 16 x 8 x 1024: scale {err[0]:.5f}, bias {err[1]:.5f}")
    # (the quadrature integrates what it should: scale + bias is the directional albedo of a white F0, 1 where nothing is masked)
    assert abs(want[0, -1].sum() - 1.0) < 2e-3
    assert err[0] <= 2 * MEASURED_QUADRATURE[0] and err[1] <= 2 * MEASURED_QUADRATURE[1]


def test_against_the_shipped_file(host_luts):
    """128 x 32 x 1024 against tests/golden/assets/PreintegratedGF.dds over every texel with x >= 8 - every texel with x >= 8 and y >= 2
    among them: the columns towards NoV = 0, where Monte-Carlo tables differ, are left out, 6.25 % of the texels (at most 10 % may be).
    Over x >= 8 and y >= 2 alone the means are 0.00557 and 0.00033 and the largest differences the same."""
    from unclerenderer_amd import assets
    shipped = assets.load_brdf_lut_dds(ROOT / "tests" / "golden" / "assets" / "PreintegratedGF.dds")
    assert shipped.shape == (32, 128, 2)
    kept = np.zeros((32, 128), bool)
    kept[:, 8:] = True
    assert 1 - kept.mean() <= 0.10
    d = np.abs(host_luts[(128, 32, 1024)].astype(np.float64) - shipped.astype(np.float64))[kept] / 65535
    mean, worst = d.mean(axis=0), d.max(axis=0)
    print(f"against the shipped file: mean scale {mean[0]:.5f}, bias {mean[1]:.5f}; largest scale {worst[0]:.5f}, bias {worst[1]:.5f}")
    for c in range(2):
        assert mean[c] <= 2 * MEASURED_SHIPPED_MEAN[c] and worst[c] <= 2 * MEASURED_SHIPPED_MAX[c]


def test_scale_plus_bias_is_at_most_one(host_luts):
    for key, lut in host_luts.items():
        assert (lut.astype(np.int64).sum(axis=-1) <= 65536).all(), key


@pytest.mark.parametrize("planted", [dict(swap=True), dict(alpha_is_roughness=True), dict(nol_test=False)], ids=["axes-exchanged", "alpha-is-roughness", "no-NoL-test"])
def test_planted_errors_change_bytes(host_luts, planted):
    from unclerenderer_amd import hostmath
    table = hostmath.brdf_lut_table(8, 64)
    assert np.array_equal(host_luts[(8, 8, 64)], R.lut32(table, 8, 8, 64))
    assert not np.array_equal(host_luts[(8, 8, 64)], R.lut32(table, 8, 8, 64, **planted))
