"""The sky capture without a GPU: ur_host_env_sky - the functions the kernel runs - against hand-worked answers, byte
for byte against the numpy fp32 restatement of tests/env_sky_ref.py, against the same rule in float64, against the float64 restatement of
the shader (tests/lighting_ref64.apply_atmosphere), its orientation, and the planted errors, which each change bytes."""
import math

import numpy as np
import pytest

from tests import env_sky_ref as R
from tests import lighting_ref64 as L64

SUNS = [(0.3, 0.8, -0.5), (0.0, -1.0, 0.0), (-40.0, 2.0, 9.0), (0.6, 0.0, 0.8)]
HEIGHTS = [1.5, 2500.0]
EDGES = [1, 2, 4, 8, 16, 32]
TAPS = [1, 2, 4, 8, 16]
# measured here over every case below: the largest |host - float64 rule| in fp16 ulps of the float64 value is 0.5010;
# the bound is twice that
MEASURED_ULPS = 0.5010


def half(v):
    return int(np.float16(v).view(np.uint16))


def test_hand_worked_answers(urlib):
    """E = 1, one tap: the +Y texel looks at the zenith, the -Y texel at the nadir. By hand, with k = 3 / (16 * 3.14159265) = 0.0596831:
    sun at the zenith, camera on the ground, no light colour: zenith = 0.05 + 0.650 k (1 + 1) = 0.127588, 0.12 + 0.570 k 2 = 0.188039,
    0.22 + 0.475 k 2 = 0.276699; nadir (falloff 1, cos -1) = horizon + the same scatter = 0.597588, 0.748039, 0.916699.
    With LightColor 1 the zenith texel looks into the sun: the Mie peak 1 / (1 - 0.76)^3 = 72.3380 times 0.8 (1 - 0.5776) / (4 pi) =
    0.0268907 adds 1.945219. A sun at the nadir dims all scatter by exp(-4) = 0.0183156: zenith red = 0.05 + 0.077588 * 0.0183156 = 0.051421."""
    from unclerenderer_amd import hostmath
    k = 3.0 / (16.0 * 3.14159265)
    up = hostmath.env_sky(R.sky_constants((0, 5, 0), (0, 0, 0), 0.0), 1, 1)
    assert up.shape == (6, 1, 1, 4) and (up[..., 3] == 0x3C00).all()
    assert list(up[2, 0, 0, :3]) == [half(0.05 + 0.650 * k * 2), half(0.12 + 0.570 * k * 2), half(0.22 + 0.475 * k * 2)] == [half(0.127588), half(0.188039), half(0.276699)]
    assert list(up[3, 0, 0, :3]) == [half(0.597588), half(0.748039), half(0.916699)]
    lit = hostmath.env_sky(R.sky_constants((0, 5, 0), (1, 1, 1), 0.0), 1, 1)
    peak = 0.8 * (1 - 0.76 ** 2) / (4 * 3.14159265) / (1 - 0.76) ** 3
    assert abs(peak - 1.945219) < 1e-5
    assert list(lit[2, 0, 0, :3]) == [half(0.127588 + peak), half(0.188039 + peak), half(0.276699 + peak)]
    down = hostmath.env_sky(R.sky_constants((0, -1, 0), (0, 0, 0), 0.0), 1, 1)
    assert down[2, 0, 0, 0] == half(0.05 + 0.650 * k * 2 * math.exp(-4.0)) == half(0.051421)
    # a camera below the ground is a camera on the ground; one 8000 m up sees 1 / e of the Rayleigh scatter
    for sun in SUNS:
        assert np.array_equal(hostmath.env_sky(R.sky_constants(sun, camera_y=-30.0), 4, 2), hostmath.env_sky(R.sky_constants(sun, camera_y=0.0), 4, 2))
    high = hostmath.env_sky(R.sky_constants((0, 5, 0), (0, 0, 0), 8000.0), 1, 1)
    assert high[2, 0, 0, 0] == half(0.05 + 0.650 * k * 2 / math.e)


def test_folded_values(urlib):
    """ur_host_env_sky_params is the float64 fold, each value rounded once."""
    from unclerenderer_amd import hostmath
    for sun in SUNS:
        for h in HEIGHTS + [-3.0]:
            sky = R.sky_constants(sun, camera_y=h)
            want = np.concatenate([np.ravel(v) for v in R.fold64(sky)]).astype(np.float32)
            got = hostmath.env_sky_params(sky)
            assert got.dtype == np.float32 and got.shape == (10,)
            # (exp and the divide in another library's double may differ in the last bit of the double: at most one fp32 ulp here)
            assert (np.abs(got.astype(np.float64) - want) <= np.spacing(np.abs(want))).all(), (sun, h, got, want)
    p = hostmath.env_sky_params(R.sky_constants((0, 5, 0), (1, 2, 4), 0.0))
    assert list(p[:3]) == [0, 1, 0] and p[9] == 1 and p[7] == np.float32(2 * float(p[6])) and p[8] == np.float32(4 * float(p[6]))


def test_without_light_colour_the_sky_is_the_same_all_around(urlib):
    """LightColor = 0 and the sun at the zenith: the colour depends on the height alone. Faces that share their normalisation's order are
    mirror images to the bit; the others agree within an fp16 ulp; the +Y face is symmetric."""
    from unclerenderer_amd import hostmath
    cube = hostmath.env_sky(R.sky_constants((0, 1, 0), (0, 0, 0), 0.0), 16, 2)
    assert np.array_equal(cube[0], cube[1][:, ::-1]) and np.array_equal(cube[4], cube[5][:, ::-1])
    v = R.cube_of(cube)
    assert (np.abs(v[0] - v[4]) <= R.half_ulp(v[4])).all()
    assert np.array_equal(cube[2], cube[2][::-1, ::-1]) and np.array_equal(cube[2], cube[2].transpose(1, 0, 2))


@pytest.mark.parametrize("E", EDGES)
def test_host_bytes_are_the_numpy_restatement(urlib, E):
    from unclerenderer_amd import hostmath
    for K in TAPS:
        for sun in SUNS:
            for h in HEIGHTS:
                sky = R.sky_constants(sun, camera_y=h)
                got = hostmath.env_sky(sky, E, K)
                want = R.capture32(tuple(np.split(hostmath.env_sky_params(sky), [3, 6, 9])), E, K)
                same = got == want
                assert same.all(), f"E {E}, K {K}, sun {sun}, height {h}: {np.count_nonzero(~same)} values differ, first at {tuple(np.argwhere(~same)[0])}"


def test_the_rule_in_float64(urlib):
    """Every texel of every case against the rule in float64 with unrounded constants: the error is the rounding to fp16 and the fp32
    arithmetic in front of it. The bound is twice the measured value."""
    from unclerenderer_amd import hostmath
    worst = 0.0
    for E in EDGES:
        for K in TAPS:
            for sun in SUNS:
                for h in HEIGHTS:
                    sky = R.sky_constants(sun, camera_y=h)
                    want = R.capture64(R.fold64(sky), E, K)
                    err = np.abs(R.cube_of(hostmath.env_sky(sky, E, K)) - want) / R.half_ulp(want)
                    worst = max(worst, float(err.max()))
    print(f"largest error against the float64 rule: {worst:.4f} fp16 ulps")
    assert worst <= 2 * MEASURED_ULPS


@pytest.mark.parametrize("E", EDGES)
def test_one_tap_is_the_shader_at_the_texel_centre(urlib, E):
    """taps = 1: every texel within one fp16 ulp of tests/lighting_ref64.apply_atmosphere at the texel centre's direction."""
    from unclerenderer_amd import hostmath
    d = R.directions(E, 1, np.float64).reshape(-1, 3)
    for sun in SUNS:
        for h in HEIGHTS + [-5.0]:
            sky = R.sky_constants(sun, camera_y=h)
            want = L64.apply_atmosphere(sky, d).reshape(6, E, E, 3)
            got = R.cube_of(hostmath.env_sky(sky, E, 1))
            assert (np.abs(got - want) <= R.half_ulp(want)).all(), (E, sun, h, float((np.abs(got - want) / R.half_ulp(want)).max()))


def face_place(d, E):
    """ur_cube::cube_face: the face and the texel coordinates (fractional) of a direction."""
    ax = np.abs(d)
    if ax[2] >= ax[0] and ax[2] >= ax[1]:
        face, ma, sc, tc = (4 if d[2] >= 0 else 5), ax[2], (d[0] if d[2] >= 0 else -d[0]), -d[1]
    elif ax[1] >= ax[0]:
        face, ma, sc, tc = (2 if d[1] >= 0 else 3), ax[1], d[0], (d[2] if d[1] >= 0 else -d[2])
    else:
        face, ma, sc, tc = (0 if d[0] >= 0 else 1), ax[0], (-d[2] if d[0] >= 0 else d[2]), -d[1]
    return face, (sc / ma + 1) / 2 * E, (tc / ma + 1) / 2 * E


@pytest.mark.parametrize("sun", [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (0.35, 0.45, -0.8)])
def test_the_brightest_texel_is_where_the_face_table_puts_the_sun(urlib, sun):
    from unclerenderer_amd import hostmath
    E = 8
    v = R.cube_of(hostmath.env_sky(R.sky_constants(sun, (30.0, 30.0, 30.0), 0.0), E, 1))[..., 0]
    face, y, x = np.unravel_index(np.argmax(v), v.shape)
    want_face, px, py = face_place(np.array(sun, np.float64), E)
    assert face == want_face and abs(x + 0.5 - px) <= 0.5 + 1e-9 and abs(y + 0.5 - py) <= 0.5 + 1e-9, (sun, (face, y, x), (want_face, py, px))


@pytest.mark.parametrize("planted", [dict(flip=(0, 2)), dict(flip=(3, 2)), dict(g_sign=-1.0), dict(exponent=2)], ids=["+X-axis-flipped", "-Y-axis-flipped", "g-sign", "falloff-exponent"])
def test_planted_errors_change_bytes(urlib, planted):
    from unclerenderer_amd import hostmath
    sky = R.sky_constants(SUNS[0])
    params = tuple(np.split(hostmath.env_sky_params(sky), [3, 6, 9]))
    got = hostmath.env_sky(sky, 8, 2)
    assert np.array_equal(got, R.capture32(params, 8, 2))
    assert not np.array_equal(got, R.capture32(params, 8, 2, **planted))
