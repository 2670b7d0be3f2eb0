"""The environment prefilter's rule without a GPU (include/ur_env_prefilter.h). ur_host_env_prefilter - the byte reference of
the device build - against hand-worked answers, against the numpy fp32 restatement of tests/env_prefilter_ref.py to the byte, against the
same rule in float64, and the restatement against the independent definition, a float64 quadrature over every texel that shares no step
with the sampler; seven planted errors, each of which must change bytes and, where the quadrature can see it, exceed its margin."""
from pathlib import Path

import numpy as np
import pytest

from tests import env_prefilter_ref as P

ASSETS = Path(__file__).parent / "golden" / "assets"
HALF_ONE = 0x3C00

# ---- the measured figures (DESIGN.md 3.20 records them; each bound is twice the measured maximum, measured on these very cubes)
# same rule in float64: fp16 ulps over the texels where float64 takes the same taps
F64_CASES = [(8, 64), (16, 64), (32, 64), (8, 1024), (16, 16)]
F64_MEASURED_ULPS = 1
F64_LEFT_OUT_CAP = 0.02
# the restatement against the quadrature, per level 1 .. L - 1, relative to the environment's mean: {(base, samples): measured maxima}
QUADRATURE_MEASURED = {
    (16, 64): (0.0105, 0.0118, 0.0170, 0.0239),
    (16, 256): (0.0077, 0.0033, 0.0048, 0.0052),
    (32, 64): (0.0093, 0.0092, 0.0124, 0.0165, 0.0280),
    (32, 256): (0.0038, 0.0024, 0.0033, 0.0041, 0.0054),
}
QUADRATURE_TEXELS = 24  # output texels a level the quadrature is evaluated at (seeded; all of a level that has fewer)
# the planted errors the quadrature must see (the others change bytes only: a smooth environment hides them)
SEEN_BY_QUADRATURE = ("alpha_r", "neg_y_tc", "no_weight", "prev_table", "unnormalised")


def host(top, base, samples):
    from unclerenderer_amd import hostmath
    raw = hostmath.env_prefilter_table(base, samples)
    return hostmath.env_prefilter(top, base, samples, table=raw), P.table_from_bytes(raw, base, samples)


def positive_cube(seed, base):
    """A seeded cube of positive values over three decades: ulps of a difference mean something (no cancellation)."""
    rng = np.random.default_rng(seed)
    return np.concatenate([0.05 + 50.0 * rng.random((6, base, base, 3)) ** 3, np.ones((6, base, base, 1))], axis=-1).astype(np.float16).view(np.uint16)


# ---- hand-worked answers
def test_edge_one_is_the_source_with_alpha_one(urlib):
    top = P.random_cube(1, 1)
    got, _ = host(top, 1, 16)
    want = top.reshape(6, 4).copy()
    want[:, 3] = HALF_ONE
    assert got.shape == (6, 4) and np.array_equal(got, want)


@pytest.mark.parametrize("base", [2, 8])
def test_constant_cube_stays_constant(urlib, base):
    """An fp16-representable colour: box means and bilinear blends of equal values are exact, and the weighted mean's fp32 error (a few
    hundred ulps of fp32 at most over 64 samples) is far below half an fp16 ulp (2^13 fp32 ulps)."""
    colour = np.array([0.337890625, 1.5, 1000.0, 7.0], np.float16).view(np.uint16)
    top = np.broadcast_to(colour, (6, base, base, 4)).copy()
    got, _ = host(top, base, 64)
    assert (got[:, :3] == colour[:3]).all() and (got[:, 3] == HALF_ONE).all()


@pytest.mark.parametrize("base", [2, 4, 16])
def test_level_zero_is_the_source(urlib, base):
    top = P.random_cube(base, base)
    got, _ = host(top, base, 16)
    want = top.copy()
    want[..., 3] = HALF_ONE
    assert np.array_equal(P.level_of_payload(got, base, 0), want)
    assert (got[:, 3] == HALF_ONE).all()


def test_table_by_hand_at_alpha_one(urlib):
    """S = 16 at the last level (r = 1, alpha = 1): cos^2 = 1 - xi2, hz = sqrt(1 - xi2), l.z = 1 - 2 xi2, D = 1 / pi. xi2 is i's bits
    mirrored: an odd i has xi2 >= 1/2 and is dropped, the even ones have xi2 = 0, 1/4, 1/8, 3/8, 1/16, 5/16, 3/16, 7/16 (i = 0, 2, .. 14):
    eight kept, sum of l.z = 8 - 2 * 1.75 = 4.5. Omega_s / Omega_p = (4 pi / 16) / (4 pi / (6 E^2)) = 6 E^2 / 16."""
    from unclerenderer_amd import hostmath
    for base in (4, 16):
        L = P.levels_of(base)
        tab = P.table_from_bytes(hostmath.env_prefilter_table(base, 16), base, 16)
        inv, kept, e = tab[L - 1]
        assert kept == 8 and inv == np.float32(1.0 / 4.5)
        xi2 = [0, 1 / 4, 1 / 8, 3 / 8, 1 / 16, 5 / 16, 3 / 16, 7 / 16]
        assert (e[1::2] == 0).all()
        assert e[0::2, 2].tolist() == [1 - 2 * x for x in xi2]
        lod = min(0.5 * np.log2(6 * base * base / 16), L - 1)
        assert (e[0::2, 3] == np.float32(lod)).all()
        i = 2  # phi = 2 pi 2 / 16 = pi / 4, xi2 = 1/4: hz = sqrt(3)/2, sin = 1/2, l.xy = 2 hz (sin cos phi, sin sin phi) = sqrt(3)/2 * sqrt(2)/2 each
        assert abs(e[i, 0] - np.sqrt(6) / 4) < 1e-7 and abs(e[i, 1] - np.sqrt(6) / 4) < 1e-7
        assert e[0].tolist()[:3] == [0, 0, 1]  # the mirror direction itself
        assert tab[0][0] == 1.0 and tab[0][1] == 0


def test_table_is_the_float64_formula(urlib):
    """Every entry of the library's table against the numpy float64 statement: the same kept samples, values within one fp32 ulp (the two
    libraries' sin, cos and log2 may differ in the last place of the double)."""
    from unclerenderer_amd import hostmath
    for base, samples in ((1, 16), (2, 16), (32, 64), (256, 1024), (2048, 4096)):
        got, want = P.table_from_bytes(hostmath.env_prefilter_table(base, samples), base, samples), P.table(base, samples)
        for k in range(1, P.levels_of(base)):
            assert got[k][1] == want[k][1] and np.array_equal(got[k][2][:, 2] > 0, want[k][2][:, 2] > 0)
            assert np.abs(got[k][2].view(np.int32).astype(np.int64) - want[k][2].view(np.int32)).max() <= 1
            assert abs(int(got[k][0].view(np.int32)) - int(want[k][0].view(np.int32))) <= 1
            assert (got[k][2][:, 3] >= 0).all() and (got[k][2][:, 3] <= P.levels_of(base) - 1).all()


def test_one_direction_and_frame_per_face():
    """Texel (x, y) = (0, 0) of a face of edge 2: s = t = -1/2. The direction by hand from the face table of DESIGN.md 3.20, over
    sqrt(1.5); the frame is orthonormal and right-handed around it."""
    n = P.directions(2, np.float64)
    h = 0.5
    by_hand = [(1, h, h), (-1, h, -h), (-h, 1, -h), (-h, -1, h), (-h, h, 1), (h, h, -1)]
    t, b = P.frame(n)
    for f in range(6):
        assert np.allclose(n[4 * f], np.array(by_hand[f]) / np.sqrt(1.5), atol=1e-15)
        assert np.allclose([n[4 * f] @ t[4 * f], n[4 * f] @ b[4 * f], t[4 * f] @ b[4 * f]], 0, atol=1e-15)
        assert np.allclose(np.cross(t[4 * f], b[4 * f]), n[4 * f], atol=1e-15)
    # the mapping is cube_face's inverse: every texel centre of an edge-8 face maps back to its own face and centre
    d = P.directions(8, np.float64)
    face, u, v = P.face_uv(d)
    centres = (np.arange(8) + 0.5) / 8
    assert np.array_equal(face, np.repeat(np.arange(6), 64))
    assert np.allclose(u.reshape(6, 8, 8), centres[None, None, :]) and np.allclose(v.reshape(6, 8, 8), centres[None, :, None])


# ---- bytes
@pytest.mark.parametrize("base,samples", [(b, s) for b in (1, 2, 4, 8, 16, 32) for s in (16, 64)] + [(8, 1024)])
def test_host_build_is_the_restatement_to_the_byte(urlib, base, samples):
    top = P.random_cube(100 * base + samples, base)
    assert np.abs(top.view(np.float16).astype(np.float32)).max() <= 60000 and np.isfinite(top.view(np.float16)).all()
    got, tab = host(top, base, samples)
    want, _ = P.prefilter(top, base, samples, tab)
    same = got == want
    assert same.all(), f"{np.count_nonzero(~same)} values differ, first at {np.argwhere(~same)[0].tolist()}"


def test_shipped_cube_block_averaged_to_edge_four(urlib):
    """The shipped cube's top level, block-averaged to 4 x 4 faces: real sky values through both implementations."""
    from unclerenderer_amd import assets
    top, base = assets.load_env_cube_top_level(ASSETS / "output_pmrem.dds")
    small = top.view(np.float16).astype(np.float64).reshape(6, 4, base // 4, 4, base // 4, 4).mean(axis=(2, 4)).astype(np.float16).view(np.uint16)
    got, tab = host(small, 4, 64)
    want, _ = P.prefilter(small, 4, 64, tab)
    assert np.array_equal(got, want) and len(np.unique(got[:, :3])) > 50


# ---- the same rule in float64
def test_same_rule_in_float64(urlib):
    """Sampling and sums in float64 over the same fp32 table. Texels where float64 takes other taps are left out; their share is capped
    (a condition on the cases: with 16 samples on small faces the Hammersley directions sit on texel boundaries, and more are left out).
    The rest agrees within twice the measured maximum of fp16 ulps."""
    worst = 0
    for base, samples in F64_CASES:
        for seed in range(3):
            top = positive_cube(1000 * seed + base + samples, base)
            tab = host(top, base, samples)[1]
            a, taps_a = P.prefilter(top, base, samples, tab, np.float32)
            b, taps_b = P.prefilter(top, base, samples, tab, np.float64)
            total = left_out = 0
            for k in range(1, P.levels_of(base)):
                other = (taps_a[k] != taps_b[k]).any(axis=(1, 2))
                la, lb = (P.level_of_payload(x, base, k).reshape(-1, 4)[:, :3].astype(np.int64) for x in (a, b))
                total, left_out = total + other.size, left_out + int(other.sum())
                if (~other).any():
                    worst = max(worst, int(np.abs(la - lb)[~other].max()))
            print(f"base {base}, {samples} samples, seed {seed}: {left_out} of {total} texels left out, worst so far {worst} ulps")
            assert left_out <= F64_LEFT_OUT_CAP * total, (base, samples, seed, left_out, total)
    assert worst <= 2 * F64_MEASURED_ULPS, worst


# ---- the independent definition, and the planted errors
@pytest.fixture(scope="module")
def smooth(urlib):
    """{(base, samples): (cube, restated chain, table, {k: (texels, quadrature)}, the environment's mean)}; the quadrature is computed once
    per base and shared."""
    out = {}
    for base in (16, 32):
        fine, w, omega, cube = P.supersampled(P.smooth_environment(5 + base), base)
        mean = float(((fine * omega[None, :, :, None]).sum(axis=(0, 1, 2)) / (6 * omega.sum())).mean())
        quad = {}
        for k in range(1, P.levels_of(base)):
            texels = 6 * (base >> k) ** 2
            chosen = np.sort(np.random.default_rng(k).choice(texels, min(texels, QUADRATURE_TEXELS), replace=False))
            quad[k] = (chosen, P.quadrature(fine, w, omega, base, k, chosen))
        for samples in (64, 256):
            got, tab = host(cube, base, samples)
            out[(base, samples)] = (cube, got, tab, quad, mean)
    return out


def errors(chain, base, quad, mean):
    """Per level 1 .. L - 1: the largest |chain - quadrature| over the chosen texels and the channels, relative to the mean."""
    out = []
    for k, (chosen, q) in quad.items():
        v = P.level_of_payload(chain, base, k).reshape(-1, 4)[chosen, :3].view(np.float16).astype(np.float64)
        out.append(float(np.abs(v - q).max() / mean))
    return out


@pytest.mark.parametrize("base,samples", sorted(QUADRATURE_MEASURED))
def test_against_the_quadrature(smooth, base, samples):
    cube, got, tab, quad, mean = smooth[(base, samples)]
    restated, _ = P.prefilter(cube, base, samples, tab)
    assert np.array_equal(restated, got)  # (what is judged is what the library computes)
    measured = errors(restated, base, quad, mean)
    print(f"base {base}, {samples} samples: per level {[round(e, 4) for e in measured]}, recorded {QUADRATURE_MEASURED[(base, samples)]}")
    for k, (e, recorded) in enumerate(zip(measured, QUADRATURE_MEASURED[(base, samples)]), 1):
        assert e <= 2 * recorded, (k, e, recorded)


@pytest.mark.parametrize("fault", P.FAULTS)
def test_planted_errors_fail(smooth, fault):
    """Each planted error changes the bytes (the byte tests fail), at every case; those the quadrature can see exceed its margin - twice
    the measured error - at some level of every case."""
    for (base, samples), (cube, got, tab, quad, mean) in smooth.items():
        wrong, _ = P.prefilter(cube, base, samples, P.table(base, samples, fault) if fault == "alpha_r" else tab, fault=fault)
        assert not np.array_equal(wrong, got), (fault, base, samples)
        e = errors(wrong, base, quad, mean)
        over = [k for k, (x, recorded) in enumerate(zip(e, QUADRATURE_MEASURED[(base, samples)]), 1) if x > 2 * recorded]
        print(f"{fault}, base {base}, {samples} samples: per level {[round(x, 4) for x in e]}, over the margin at levels {over}")
        if fault in SEEN_BY_QUADRATURE:
            assert over, (fault, base, samples, e)
    # the byte test itself sees it on a random cube too
    top = P.random_cube(5, 8)
    got, tab = host(top, 8, 64)
    wrong, _ = P.prefilter(top, 8, 64, P.table(8, 64, fault) if fault == "alpha_r" else tab, fault=fault)
    assert not np.array_equal(wrong, got)
