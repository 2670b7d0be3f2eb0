"""The Forward rule as tests/forward_ref.py restates it: answers worked out by hand on an 8 x 8 target under
depth_ref.hand_camera (power-of-two geometry: every weight is exact), the accuracy of the fp32 rule against float64 over the soups, and
planted errors that must each fail a check."""
import numpy as np
import pytest

from tests import depth_ref as D
from tests import forward_ref as FW
from tests import gbuffer_mask_ref as M
from tests import gbuffer_tex_ref as X
from tests.test_gbuffer_mask_ref import CHECKER, quad, soup_reference, texture

W = H = 8
Z = 0.25  # the quads' view depth: world (= view) x = (px + 0.5) / 16 - 0.25, y = 0.25 - (py + 0.5) / 16 at a centre
F = np.float32
NORMAL, MR, BASE, EMISSIVE, MASK = X.NORMAL, X.METALLIC_ROUGHNESS, X.BASE_COLOR, X.EMISSIVE, M.ALPHA_MASK


def constant_cube(values, base=8):
    """A cube whose mip m holds values[m] in R, G and B of every texel."""
    out = []
    for _ in range(6):
        for m, v in enumerate(values):
            n = max(1, base >> m)
            t = np.zeros((n * n, 4), np.float16)
            t[:, :3], t[:, 3] = v, 1.0
            out.append(t.view(np.uint16))
    return np.concatenate(out)


def integer_cube(seed, base=8, mips=4):
    """Small seeded integers: every bilinear blend with weights of halves and quarters is exact."""
    rng = np.random.default_rng(seed)
    n = 6 * sum(max(1, base >> m) ** 2 for m in range(mips))
    t = np.ones((n, 4), np.float16)
    t[:, :3] = rng.integers(0, 64, (n, 3))
    return t.view(np.uint16)


def constant_lut(a, b, w=128, h=32):
    return np.broadcast_to(np.array([a, b], np.uint16), (h, w, 2)).copy()


def frame(**kw):
    """The hand cases' frame: the eye at the origin, a white light of intensity 2 along -z (the quads' normal), no shadow, a cube of 1, 2,
    4, 8 per mip and a LUT of (1/4-ish, 1/2-ish): codes 16384 and 32768."""
    f = dict(camera=np.zeros(3, F), light_direction=np.array([0, 0, -3], F), light_color=np.array([1.0, 0.5, 0.25], F), light_intensity=2.0,
             lvp=np.array([8, 0, 0, 0, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0.5, 1], F), shadow_strength=0.0, shadow_bias=0.0, shadow=None,
             cube_bits=constant_cube([1.0, 2.0, 4.0, 8.0]), env_base=8, env_mips=4, lut=constant_lut(16384, 32768))
    f.update(kw)
    return FW.Frame(**f)


def closed_form(frm, normal, albedo, metallic, roughness, emissive, shadow, cube_pre, cube_irr, z=Z):
    """ForwardPS.hlsl for a plane at view depth z under hand_camera with constant material values, a constant cube colour per lookup and a
    constant LUT, written out in float64 per texel: (8, 8, 3)."""
    py, px = np.mgrid[0:8, 0:8]
    wpos = np.stack([((px + 0.5) / 4 - 1) * z, (1 - (py + 0.5) / 4) * z, np.full((8, 8), z)], -1)
    unit = lambda v: v / np.sqrt((v * v).sum(-1, keepdims=True))  # noqa: E731
    n = unit(np.broadcast_to(np.asarray(normal, np.float64), (8, 8, 3)))
    v = unit(frm.camera.astype(np.float64) - wpos)
    ld = unit(frm.light_direction.astype(np.float64))
    hv = unit(v + ld)
    sat = lambda x: np.clip(x, 0, 1)  # noqa: E731
    nl, nv, nh, vh = sat((n * ld).sum(-1)), sat((n * v).sum(-1)), sat((n * hv).sum(-1)), sat((v * hv).sum(-1))
    albedo = np.asarray(albedo, np.float64)
    f0 = 0.04 + metallic * (albedo - 0.04)
    a2 = roughness ** 4
    d = a2 / np.maximum(np.float64(F(3.14159265)) * (nh * nh * (a2 - 1) + 1) ** 2, 1e-4)
    k = (roughness + 1) ** 2 / 8
    g = nv / (nv * (1 - k) + k) * nl / (nl * (1 - k) + k)
    fr = f0 + (1 - f0) * ((1 - vh) ** 5)[..., None]
    spec = (d * g)[..., None] * fr / np.maximum(4 * nl * nv, 1e-4)[..., None]
    pbr = ((1 - fr) * (1 - metallic) * albedo + spec) * nl[..., None]
    lighting = pbr * frm.light_intensity * frm.light_color.astype(np.float64) * np.asarray(shadow, np.float64)[..., None]
    bx, by = frm.lut[0, 0].astype(np.float64) / 65535
    return lighting + cube_irr * albedo * (1 - metallic) + cube_pre * (f0 * bx + by) + np.asarray(emissive, np.float64)


def close(hdr_bits, want, what):
    """Every colour channel is one of the two fp16 neighbours of the closed form (the fp32 error is far below an fp16 ulp), alpha is 1."""
    e = FW.R.signed_error(hdr_bits[..., :3], want)
    assert np.abs(e).max() <= 1.0, (what, float(np.abs(e).max()))
    assert (hdr_bits[..., 3] == 0x3C00).all(), what


def flat_normal_map():
    t = np.zeros((8, 8, 4), np.uint8)
    t[:] = (128, 128, 255, 255)
    return X.Tex([t], False)


def _with(draw, columns, value):
    """The draw with the floats `columns` of every vertex set to `value`."""
    v = np.ascontiguousarray(draw.vertices).view(F).reshape(-1, 16).copy()
    v[:, columns] = value
    draw.vertices = v.reshape(-1).view(np.uint8).copy()
    return draw


def hand_cases():
    """name -> (draws, materials, opaque slots, masked slots, frame); the GPU test runs them too."""
    rng = np.random.default_rng(12)
    mr_tex = X.Tex([rng.integers(1, 256, (8, 8, 4), dtype=np.uint8)], False)
    base_tex = X.Tex([rng.integers(1, 256, (8, 8, 4), dtype=np.uint8)], True)
    half = np.zeros((2, 2, 4), np.uint8)
    half[:, 0], half[:, 1] = 127, 128
    shadow4 = np.tile(np.array([0, 0, 1, 1], F), (4, 1))
    edge_lvp = np.array([8, 0, 0, 0, 0, 2, 0, 0, 0, 0, 0, 0, 0.25, 0, 0.5, 1], F)
    fixed_lvp = np.array([0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0.5, 0, 0.5, 1], F)
    plain = dict(base_color=np.array([0.5, 0.25, 1.0], F), emissive=np.array([0.125, 0, 2.0], F), metallic=0.25, roughness=0.5)
    mirror = dict(base_color=np.zeros(3, F), metallic=0.0)
    lut01 = constant_lut(0, 65535)
    spot = np.array([(3 + 0.5) / 16 - 0.25, 0.25 - (4 + 0.5) / 16, Z], F)  # the centre of texel (3, 4)
    scaled = {"metallic_roughness": ((0.375, 0.25), (2.0, 3.0), (0.0, 1.0))}
    tri = M.MaskDraw(np.concatenate([np.array(D.at(x, y, Z, W, H) + [0, 0, -1, 0, 0, 1, 0, 0, 1, 1, 1, 1, 1], F) for x, y in ((0, 0), (0, 8), (8, 0))]).view(np.uint8).copy(),
                     np.arange(3, dtype=np.uint32), **plain)
    return {
        "flat_normal_map": ([quad(Z, **plain)], [{"key": NORMAL, "normal": flat_normal_map()}], [0], [], frame()),
        "shadow_window": ([quad(Z, **plain)], [{"key": 0}], [0], [], frame(shadow_strength=0.75, shadow_bias=0.25, shadow=shadow4, cube_bits=constant_cube([0, 0, 0, 0]))),
        "shadow_edge": ([quad(Z, **plain)], [{"key": 0}], [0], [], frame(shadow_strength=0.75, shadow_bias=0.25, shadow=np.zeros((4, 4), F), lvp=edge_lvp)),
        "shadow_2x2": ([quad(Z, **plain)], [{"key": 0}], [0], [], frame(shadow_strength=1.0, shadow_bias=0.25, shadow=np.zeros((2, 2), F), lvp=fixed_lvp)),
        "roughness_0": ([quad(Z, **dict(plain, roughness=0.0))], [{"key": 0}], [0], [], frame()),
        "roughness_1": ([quad(Z, **dict(plain, roughness=1.0))], [{"key": 0}], [0], [], frame()),
        "cube_edge": ([quad(Z, roughness=0.0, **mirror)], [{"key": 0}], [0], [], frame(camera=spot + F([2, 0, -2]), light_intensity=0.0, cube_bits=integer_cube(3), lut=lut01)),
        "cube_corner": ([quad(Z, roughness=0.0, **mirror)], [{"key": 0}], [0], [], frame(camera=spot + F([2, 2, -2]), light_intensity=0.0, cube_bits=integer_cube(4), lut=lut01)),
        "degenerate_tangent_normal": ([_with(quad(Z, **plain), slice(6, 8), 0.5)], [{"key": NORMAL, "normal": X.Tex([half], False)}], [0], [], frame()),
        "zero_normal": ([_with(quad(Z, **plain), slice(3, 6), 0.0)], [{"key": 0}], [0], [], frame()),
        "half_covered": ([tri], [{"key": 0}], [0], [], frame()),
        "masked_hole": ([quad(Z, **plain)], [{"key": MASK | BASE, "base_color": texture(CHECKER)}], [], [0], frame()),
        "mr_at_base_uv": ([quad(Z, transforms=scaled, **plain)], [{"key": MR | BASE, "metallic_roughness": mr_tex, "base_color": base_tex}], [0], [], frame()),
    }


def background():
    """The HDR in front of the pass: a seeded image (what the sky drew)."""
    return np.random.default_rng(7).integers(0, 0x7800, (H, W, 4)).astype(np.uint16)


def run_case(name, flags=0, precise=False, plant=None, case=None):
    draws, mats, opaque, masked, frm = hand_cases()[name] if case is None else case
    cam = D.hand_camera(W, H)
    depth, _ = D.depth_prepass(draws, *cam, W, H, flags=flags, slots=opaque)
    out = FW.forward_pass(draws, *cam, depth, W, H, frm, materials=mats, flags=flags, select=[(s, s) for s in opaque], mask_select=[(s, s) for s in masked],
                          hdr=background(), precise=precise, plant=plant)
    return out, depth, frm


PLAIN = dict(albedo=[0.5, 0.25, 1.0], metallic=0.25, roughness=0.5, emissive=[0.125, 0, 2.0])


def test_flat_normal_map_under_a_light_along_the_normal():
    """Texel (128, 128, 255): the tangent normal (1/255, 1/255, 1) in the frame T = (1, 0, 0), B = (0, -1, 0), N = (0, 0, -1). Roughness 1/2
    with four mips is level 1.5: the prefiltered colour is (2 + 4) / 2, irradiance the last mip's 8."""
    out, _, frm = run_case("flat_normal_map")
    d = 1.0 / 255.0
    close(out["hdr"], closed_form(frm, [d, -d, -1.0], shadow=np.ones((8, 8)), cube_pre=3.0, cube_irr=8.0, **PLAIN), "flat normal map")
    assert (out["keys"] != 0).all()


def test_shadow_window_half_inside():
    """shadowUV.x = (px + 0.5) / 4 - 0.5: columns 2-5 lie in the window of a 4 x 4 map whose columns are (0, 0, 1, 1) against a compare value
    of 1/4; the four taps half a texel off the centres of columns 0-3 give PCF 1/4, 1/4, 3/4, 1 (the white border right of column 3)."""
    out, _, frm = run_case("shadow_window")
    pcf = np.array([1, 1, 0.25, 0.25, 0.75, 1, 1, 1])
    shadow = np.tile(1 + 0.75 * (pcf - 1), (8, 1))
    want = closed_form(frm, [0, 0, -1.0], shadow=shadow, cube_pre=0.0, cube_irr=0.0, **PLAIN)
    close(out["hdr"], want, "shadow window")
    lit = closed_form(frm, [0, 0, -1.0], shadow=np.ones((8, 8)), cube_pre=0.0, cube_irr=0.0, **PLAIN)
    assert np.abs(want - lit)[:, 2:5].min() > 0.01  # the check above tells the columns apart


def test_texel_on_the_shadow_window_edge_is_inside():
    """shadowUV.x = (px + 0.5) / 4 - 0.375 is exactly 1 in column 5 and exactly 0 in column 1: both inside; columns 0, 6 and 7 are outside."""
    out, _, frm = run_case("shadow_edge")
    suv, _, inside = FW.shadow_coordinates(out["material32"], frm, F)
    assert (suv.reshape(8, 8, 2)[:, 5, 0] == 1.0).all() and inside.reshape(8, 8)[:, 5].all() and not inside.reshape(8, 8)[:, 6].any()
    # columns 1-5 are inside (column 1 at exactly 0). Taps at u * 4 - 0.5 for u = x -+ 1/8 over a map of zeros: column 1 reads the border
    # left of the map (1) and texel 0 with weight 1; columns 2-4 whole texels of the map; column 5 texel 3 and the border right of it
    pcf = np.array([1, 0.5, 0, 0, 0, 0.5, 1, 1])
    shadow = np.tile(1 + 0.75 * (pcf - 1), (8, 1))
    close(out["hdr"], closed_form(frm, [0, 0, -1.0], shadow=shadow, cube_pre=3.0, cube_irr=8.0, **PLAIN), "shadow edge")


def test_two_by_two_shadow_map():
    """shadowUV = (3/4, 1/2) everywhere over a 2 x 2 map of zeros: the taps at x = 3/4 +- 1/4 read columns (1, border) half and half, and
    columns (0, 1): PCF 1/4, and full strength leaves a quarter of the light."""
    out, _, frm = run_case("shadow_2x2")
    close(out["hdr"], closed_form(frm, [0, 0, -1.0], shadow=np.full((8, 8), 0.25), cube_pre=3.0, cube_irr=8.0, **PLAIN), "2 x 2 shadow map")


def test_roughness_0_and_1_read_one_mip():
    out, _, frm = run_case("roughness_0")
    close(out["hdr"], closed_form(frm, [0, 0, -1.0], shadow=np.ones((8, 8)), cube_pre=1.0, cube_irr=8.0, **dict(PLAIN, roughness=0.0)), "roughness 0")
    out, _, frm = run_case("roughness_1")
    close(out["hdr"], closed_form(frm, [0, 0, -1.0], shadow=np.ones((8, 8)), cube_pre=8.0, cube_irr=8.0, **dict(PLAIN, roughness=1.0)), "roughness 1")


@pytest.mark.parametrize("name,tie", [("cube_edge", 2), ("cube_corner", 3)])
def test_reflection_on_a_cube_edge_and_corner(name, tie):
    """The eye sits diagonally off texel (3, 4)'s centre: V = (a, 0, -a) or (b, b, -b), and reflect(-V, (0, 0, -1)) = (-a, 0, -a) or
    (-b, -b, -b) exactly: two or three equal |components|, face -Z by the tie rule, u = 1 (and v = 1). A black dielectric under a light of
    intensity 0 with a LUT of (0, 1) stores the prefiltered sample itself: the mean of four bordered texels, two or three of them another
    face's (integers: every blend is exact)."""
    out, _, frm = run_case(name)
    m = out["material32"]
    at = 4 * 8 + 3
    toeye = (frm.camera - m["wpos"][at])[None]
    v = toeye / np.sqrt(FW._dot(toeye, toeye))
    r = -v - (F(2) * FW._dot(-v, m["n"][at:at + 1]))[:, None] * m["n"][at:at + 1]
    assert (np.abs(r[0]) == np.abs(r[0, 2])).sum() == tie and r[0, 2] < 0
    face, u, vv = FW.cube_face32(r)
    assert face[0] == 5 and u[0] == 1.0 and vv[0] == (1.0 if tie == 3 else 0.5)
    tab, n = frm.env.fold[0], 8
    j0 = 8 if tie == 3 else 4
    idx = [tab[5, j0, 8], tab[5, j0, 9], tab[5, j0 + 1, 8], tab[5, j0 + 1, 9]]
    stride = sum(max(1, n >> k) ** 2 for k in range(4))  # texels of one face's chain
    assert sum(i // stride != 5 for i in idx) == (3 if tie == 3 else 2)
    want = frm.env.texels[idx].mean(axis=0)
    got = out["hdr"][4, 3].view(np.float16).astype(np.float64)
    assert np.array_equal(got[:3], want) and got[3] == 1.0


def test_degenerate_tangent_normal_takes_0_0_1():
    """TEXCOORD (1/2, 1/2) everywhere: the sample is the mean of the 2 x 2 texels. The map's mean is 127.5 / 255 within an fp32 ulp in every channel: the tangent normal is shorter than 1e-5, (0, 0, 1) stands in,
    and the world normal is the vertex normal: the bytes of the same draw without a normal map."""
    out, _, frm = run_case("degenerate_tangent_normal")
    case = list(hand_cases()["degenerate_tangent_normal"])
    case[1] = [{"key": 0}]
    bare, _, _ = run_case("none", case=tuple(case))
    nm = out["material32"]
    assert np.array_equal(nm["n"], np.tile(F([0, 0, -1]), (64, 1))) and (nm["bits"] == NORMAL).all()
    assert np.array_equal(out["hdr"], bare["hdr"])
    close(out["hdr"], closed_form(frm, [0, 0, -1.0], shadow=np.ones((8, 8)), cube_pre=3.0, cube_irr=8.0, **PLAIN), "degenerate tangent normal")


def test_zero_normal_is_nan_as_normalize_makes_it():
    out, _, _ = run_case("zero_normal")
    h = out["hdr"].view(np.float16)
    assert np.isnan(h[..., :3]).all() and (out["hdr"][..., 3] == 0x3C00).all()


def test_key_0_texels_keep_their_hdr():
    out, _, frm = run_case("half_covered")
    covered = out["keys"] != 0
    assert 20 < covered.sum() < 40
    assert np.array_equal(out["hdr"][~covered], background()[~covered])
    close(out["hdr"][covered], closed_form(frm, [0, 0, -1.0], shadow=np.ones((8, 8)), cube_pre=3.0, cube_irr=8.0, **PLAIN)[covered], "half covered")


def test_masked_hole_shows_the_hdr_behind():
    """The checkerboard of section 3.11: discarded texels keep key 0 and the background, the others are shaded with the texture's white."""
    out, depth, frm = run_case("masked_hole")
    even = np.fromfunction(lambda y, x: (x + y) % 2 == 0, (8, 8))
    assert np.array_equal(out["keys"] != 0, even) and out["won"] == 32 and np.array_equal(out["depth"], np.where(even, F(0.5), F(0)))
    assert np.array_equal(out["hdr"][~even], background()[~even])
    close(out["hdr"][even], closed_form(frm, [0, 0, -1.0], shadow=np.ones((8, 8)), cube_pre=3.0, cube_irr=8.0, **PLAIN)[even], "masked hole")


def test_metallic_roughness_is_sampled_at_base_uv():
    """One texel per pixel at the base-colour transform (identity): metallic and roughness are the factors times B and G of texel (px, py),
    whatever MetallicRoughnessTransform says; sampling at that transform instead (the base pass' way) gives other values."""
    out, _, _ = run_case("mr_at_base_uv")
    tex = hand_cases()["mr_at_base_uv"][1][0]["metallic_roughness"].levels[0]
    m = out["material32"]
    unorm = (np.arange(256, dtype=F) / F(255.0)).astype(F)
    assert np.array_equal(m["roughness"].reshape(8, 8), F(0.5) * unorm[tex[:, :, 1]]) and np.array_equal(m["metallic"].reshape(8, 8), F(0.25) * unorm[tex[:, :, 2]])
    planted, _, _ = run_case("mr_at_base_uv", plant="mr_transform")
    assert not np.array_equal(planted["material32"]["roughness"], m["roughness"]) and not np.array_equal(planted["hdr"], out["hdr"])


def test_f0_is_0_04_not_the_g_buffer_value():
    """A black dielectric under no light with a cube of 2 and a LUT of (32785 / 65535, 0) stores 2 * 0.04 * 0.50027: 1311.42 units of
    2^-15, code 1311. With spec0 as the G-buffer holds it (fp16 0.04 = 1311 x 2^-15) the product is 1311.70 units: code 1312."""
    case = ([quad(Z, base_color=np.zeros(3, F), metallic=0.0, roughness=0.0)], [{"key": 0}], [0], [],
            frame(light_intensity=0.0, cube_bits=constant_cube([2.0, 2.0, 2.0, 0.0]), lut=constant_lut(32785, 0)))
    code = 0x2800 + (1311 - 1024)  # 2^-5 <= x < 2^-4: exponent field 10, mantissa x / 2^-15 - 1024
    out, _, _ = run_case("none", case=case)
    assert (out["hdr"][..., :3] == code).all()
    planted, _, _ = run_case("none", case=case, plant="spec0")
    assert (planted["hdr"][..., :3] == code + 1).all()


# ---- the soups -----------------------------------------------------------------------------------------------------------------------------

_SOUP = {}


def forward_soup(w, h, seed):
    """(draws, materials, opaque, masked, view, projection, depth, frame, precise result) of a soup, computed once and left unchanged."""
    key = (w, h, seed)
    if key not in _SOUP:
        draws, mats, opaque, masked, view, proj, depth, _ = soup_reference(w, h, seed)
        frm = FW.soup_frame(w, h, seed)
        out = FW.forward_pass(draws, view, proj, depth, w, h, frm, materials=mats, select=opaque, mask_select=masked, precise=True)
        _SOUP[key] = (draws, mats, opaque, masked, view, proj, depth, frm, out)
    return _SOUP[key]


@pytest.mark.parametrize("w,h,seed", FW.SOUPS)
def test_soups_reach_what_they_are_for(w, h, seed):
    *_, frm, out = forward_soup(w, h, seed)
    m = out["material32"]
    _, _, inside = FW.shadow_coordinates(m, frm, F)
    level = m["roughness"] * F(frm.env_mips - 1)
    print(f"soup {w}x{h}: {inside.mean():.1%} of the shaded texels inside the shadow window, levels {level.min():.2f} .. {level.max():.2f}")
    assert 0.2 < inside.mean() < 0.9 and level.min() < 1 and level.max() > 2
    assert set(np.unique(m["bits"]).tolist()) == set(range(16))
    assert set(FW.cube_face32(m["n"])[0].tolist()) == set(range(6))


@pytest.mark.parametrize("w,h,seed", FW.SOUPS)
def test_soups_accuracy_against_float64(w, h, seed):
    *_, out = forward_soup(w, h, seed)
    left_out, ulps = FW.accuracy(out)
    print(f"soup {w}x{h}: {left_out:.3%} of the shaded texels left out, HDR within {ulps:.4f} fp16 ulps of float64")
    assert left_out <= 0.02
    assert ulps <= FW.ULPS_BOUND
    assert FW.ULPS_BOUND == 2.0 ** np.ceil(np.log2(2 * FW.MEASURED_ULPS)) and (ulps <= FW.MEASURED_ULPS + 1e-4)


@pytest.mark.parametrize("plant", ["mr_transform", "raw_tangent", "view_normal"])
def test_planted_errors_miss_the_bound(plant):
    w, h, seed = FW.SOUPS[0]
    draws, mats, opaque, masked, view, proj, depth, frm, out = forward_soup(w, h, seed)
    planted = FW.forward_pass(draws, view, proj, depth, w, h, frm, materials=mats, select=opaque, mask_select=masked, plant=plant)
    planted.update({k: out[k] for k in ("color64", "fragile", "same", "differs")})
    _, ulps = FW.accuracy(planted)
    print(f"{plant}: {ulps:.1f} fp16 ulps")
    assert ulps > FW.ULPS_BOUND
