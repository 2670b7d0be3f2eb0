"""The textured GBuffer rule as tests/gbuffer_tex_ref.py restates it: answers worked out by hand on an 8 x 8
target under depth_ref.hand_camera, the two host tables, the level of detail against float64, the soups' coverage conditions and the
accuracy of the fp32 rule against float64."""
import numpy as np
import pytest

from tests import depth_ref as D
from tests import gbuffer_ref as G
from tests import gbuffer_tex_ref as X

W = H = 8


def _quad(uv_of, z=0.25, tangent=(1, 0, 0, 1), **kw):
    """The screen-filling quad of tests/test_gbuffer_ref.py at view depth z with TEXCOORD uv_of(X, Y) at a corner (X, Y) of the target."""
    corners = [(0, 0), (0, 8), (8, 0), (8, 0), (0, 8), (8, 8)]
    v = np.zeros((6, 16), np.float32)
    for k, (x, y) in enumerate(corners):
        v[k, 0:3] = D.at(x, y, z, W, H)
        v[k, 3:6] = (0, 0, -1)
        v[k, 6:8] = uv_of(x, y)
        v[k, 8:12] = tangent
        v[k, 12:16] = 1.0
    return X.TexDraw(v.reshape(-1).view(np.uint8).copy(), np.arange(6, dtype=np.uint32), **kw)


def _ramp(w, h, mips=1):
    """Texel (x, y) of level k holds R = 16 x + y + 32 k, G = 255 - R, B = x, A = 255: every texel of every level differs."""
    out = []
    for k in range(mips):
        hk, wk = max(1, h >> k), max(1, w >> k)
        y, x = np.mgrid[0:hk, 0:wk]
        r = (16 * x + y + 32 * k).astype(np.uint8)
        out.append(np.stack([r, 255 - r, x.astype(np.uint8), np.full_like(r, 255)], axis=2))
    return out


def hand_cases():
    """name -> (draws, materials); the GPU test runs them too."""
    tex8 = X.Tex(_ramp(8, 8))
    cases = {}
    # one texel per pixel, centres on centres: the sample is the texel under the pixel; stretching u by N keeps L = 0 (rho^2 = Pmax^2 / N^2 = 1)
    for n in (1, 2, 3, 4):
        wide = X.Tex(_ramp(8 * n if n != 3 else 24, 8))
        cases[f"integer_scale_n{n}"] = ([_quad(lambda x, y: (x / 8.0, y / 8.0), emissive=np.float32([1, 1, 1]))],
                                        [{"key": X.EMISSIVE, "emissive": wide}])
    cases["minify_2_to_1"] = ([_quad(lambda x, y: (x / 4.0, y / 4.0), emissive=np.float32([1, 1, 1]))],
                              [{"key": X.EMISSIVE, "emissive": X.Tex(_ramp(8, 8, 2))}])
    cases["wrap_seam"] = ([_quad(lambda x, y: (x / 8.0 + 0.4375, y / 8.0 - 3.0625), emissive=np.float32([1, 1, 1]))],
                          [{"key": X.EMISSIVE, "emissive": tex8}])
    cases["rotated_transform"] = ([_quad(lambda x, y: (x / 8.0, y / 8.0), emissive=np.float32([1, 1, 1]),
                                         transforms={"emissive": ((1.0, 0.0), (1.0, 1.0), (0.0, 1.0))})],
                                  [{"key": X.EMISSIVE, "emissive": tex8}])
    flat = X.Tex([np.full((4, 4, 4), 128, np.uint8)])
    cases["flat_normal_map"] = ([_quad(lambda x, y: (x / 8.0, y / 8.0))], [{"key": X.NORMAL, "normal": flat}])
    cases["all_maps"] = ([_quad(lambda x, y: (x / 2.0, y / 3.0), base_color=np.float32([0.5, 0.25, 1.0]), emissive=np.float32([1, 2, 3]), metallic=0.5, roughness=0.75)],
                         [{"key": 15, "base_color": X.Tex(_ramp(16, 16, 5), True), "metallic_roughness": X.Tex(_ramp(13, 7, 4)), "normal": X.Tex(_ramp(8, 4)),
                           "emissive": X.Tex(_ramp(1, 1), True)}])
    # ---- the sampler at the ends of its declared ranges (rule 6's non-finite coordinate, the 2^30 limit, chains of up to 255 levels)
    one = np.float32([1, 1, 1])
    emissive = lambda tex: [{"key": X.EMISSIVE, "emissive": tex}]  # noqa: E731
    nan, inf = float("nan"), float("inf")
    ramp4 = X.Tex(_ramp(8, 8, 4))
    nan_u = lambda x, y: (nan if (x, y) == (8, 0) else x / 8.0, y / 8.0)  # noqa: E731 (the corner both triangles share)
    cases["nan_u_one_level"] = ([_quad(nan_u, emissive=one)], emissive(tex8))
    cases["nan_u_four_levels"] = ([_quad(nan_u, emissive=one)], emissive(ramp4))
    cases["inf_v"] = ([_quad(lambda x, y: (x / 8.0, inf), emissive=one)], emissive(ramp4))
    cases["nan_uv"] = ([_quad(lambda x, y: (nan, nan), emissive=one)], emissive(ramp4))
    for name, u in boundary_coordinates().items():
        cases[f"limit_{name}"] = ([_quad(lambda x, y: (0.0, 0.0), emissive=one, transforms={"emissive": ((u, 0.5), (1.0, 1.0), (1.0, 0.0))})],
                                  emissive(X.Tex(_ramp(*BOUNDARY_SHAPE))))
    for name, g in (("huge_gradient", 2.0 ** 26), ("huge_gradient_past_limit", 2.0 ** 28)):
        cases[name] = ([_quad(lambda x, y, g=g: (x * g, y * g), emissive=one)], emissive(ramp4))
    for mips in CHAIN_MIPS:
        cases[f"chain{mips}_nan"] = ([_quad(lambda x, y: (nan, nan), emissive=one)], emissive(chain_texture(mips)))
    for mips, g, _ in CHAIN_GRADIENTS:
        cases[f"chain{mips}_gradient_2p{int(np.log2(g))}"] = ([_quad(lambda x, y, g=g: (x * g, y * g), emissive=one)], emissive(chain_texture(mips)))
    return cases


BOUNDARY_SHAPE = (13, 7)  # 2^30 mod 13 = 12: a kept and a dropped coordinate land on different texels
CHAIN_MIPS = (17, 33, 40, 255)
# (mips, TEXCOORD gradient per pixel g, the level d it selects): on the 12 x 10 base Px = 12 g, Py = 10 g, N = 2, rho = 6 g, so
# L = floor(256 (log2 g + log2 6)) = floor(256 (log2 g + 2.58496)): g = 2^30 gives 8341 (d = 32, f = 149 / 256), g = 2^33 gives 9109 (d = 35)
CHAIN_GRADIENTS = ((17, 2.0 ** 30, 16), (33, 2.0 ** 30, 32), (40, 2.0 ** 30, 32), (255, 2.0 ** 30, 32), (40, 2.0 ** 33, 35))


def chain_texture(mips):
    """A 12 x 10 base with 5 real levels (12 x 10, 6 x 5, 3 x 2, 1 x 1, 1 x 1); every level behind them is 1 x 1 too, each with its own
    random texel. The base is wider than one texel: a level shift that wraps its count would take a deep level for 12 x 10."""
    return X.random_texture(12, 10, mips, False, np.random.default_rng(77))


def boundary_coordinates():
    """By search in fp32, the u whose x = fl(fl(u * 13) - 0.5) is the largest value with |x| <= 2^30 (`kept`) and the next u up
    (`dropped`), and their mirror images. The coordinate rides in the texture transform's offset over TEXCOORD (0, 0) at every vertex:
    0 * scale * rotation + offset is the offset exactly, where (b0 u + b1 u) + b2 u of three equal TEXCOORDs is u only to an ulp."""
    size = np.float32(BOUNDARY_SHAPE[0])
    x_of = lambda u: np.float32(np.float32(u * size) - np.float32(0.5))  # noqa: E731
    u = np.float32(2.0 ** 30 / 13.0)
    while abs(x_of(u)) <= X.COORD_LIMIT:
        u = np.nextafter(u, np.float32(np.inf))
    while abs(x_of(u)) > X.COORD_LIMIT:
        u = np.nextafter(u, np.float32(0))
    kept, dropped = u, np.nextafter(u, np.float32(np.inf))
    assert abs(x_of(kept)) <= X.COORD_LIMIT < abs(x_of(dropped))
    return {"kept_positive": float(kept), "dropped_positive": float(dropped), "kept_negative": float(-kept), "dropped_negative": float(-dropped)}


def _run(name, flags=0):
    draws, mats = hand_cases()[name]
    cam = D.hand_camera(W, H)
    depth, _ = D.depth_prepass(draws, *cam, W, H, flags=flags)
    return X.gbuffer_pass(draws, *cam, depth, W, H, materials=mats, flags=flags)


def _emissive(out):
    return out["hdr"].view(np.float16).astype(np.float64)[:, :, :3]


def _info(out, name="emissive"):
    rows, N, L, taps, _ = out["shade32"]["info"][name][0]
    return N, L


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_integer_texel_scale_returns_the_texel_at_each_probe_count(n):
    """u spans n x 8 texels over 8 pixels, v 8 over 8: Px = n, Py = 1, N = n, rho = 1, L = 0. The probes sit at the centres of the n
    texels under the pixel (n = 3: offsets of a third of 3 texels), so the sample is their mean: R = 16 (n px + (n - 1) / 2) + py."""
    out = _run(f"integer_scale_n{n}")
    N, L = _info(out)
    assert (N == n).all() and (L == 0).all()
    py, px = np.mgrid[0:8, 0:8]
    want = (16.0 * (n * px + (n - 1) / 2.0) + py) % 256
    if n == 1:
        want = 16.0 * px + py
        assert np.array_equal(out["hdr"][:, :, 0], (want / 255.0).astype(np.float32).astype(np.float16).view(np.uint16))
    else:
        r = np.stack([(16 * (n * px + i) + py) % 256 for i in range(n)]).mean(axis=0)
        assert np.abs(_emissive(out)[:, :, 0] - r / 255.0).max() <= 2.0 ** -10  # fp16 rounding of a value below 1, the fp32 error far below it


def test_two_to_one_minification_lands_on_level_one_exactly():
    """u, v span 16 texels over 8 pixels: rho = 2, L = 256 exactly, f = 0: only level 1 (4 x 4) is read, and a pixel centre lies on a
    texel centre of it."""
    out = _run("minify_2_to_1")
    N, L = _info(out)
    assert (N == 1).all() and (L == 256).all()
    py, px = np.mgrid[0:8, 0:8]
    want = 16 * (px % 4) + (py % 4) + 32
    assert np.array_equal(out["hdr"][:, :, 0], (want / np.float32(255.0)).astype(np.float16).view(np.uint16))


def test_wrap_seam():
    """The quad's u starts at 3.5 texels of 8 and v at -24.5: pixel centres fall between texels, columns 4 and rows 0 straddle the seam, and
    the result is the mean of four texels with true-modulo indices."""
    out = _run("wrap_seam")
    tex = _ramp(8, 8)[0][:, :, 0].astype(np.float64)
    py, px = np.mgrid[0:8, 0:8]
    x0, y0 = (px + 3) % 8, (py - 25) % 8  # floor(px + 0.5 + 3.5 - 0.5), floor(py + 0.5 - 24.5 - 0.5)
    want = (tex[y0, x0] + tex[y0, (x0 + 1) % 8] + tex[(y0 + 1) % 8, x0] + tex[(y0 + 1) % 8, (x0 + 1) % 8]) / 4.0 / 255.0
    assert np.abs(_emissive(out)[:, :, 0] - want).max() <= 2.0 ** -11


def test_uv_transform_with_rotation():
    """Rotation (cos 0, sin 1) and offset (1, 0): (u, v) -> (1 - v, u): the picture is the texture turned a quarter."""
    out = _run("rotated_transform")
    tex = _ramp(8, 8)[0][:, :, 0]
    py, px = np.mgrid[0:8, 0:8]
    want = tex[px, 7 - py]  # texel x = 8 (1 - v) - 0.5 = 7 - py, texel y = px
    assert np.array_equal(out["hdr"][:, :, 0], (want / np.float32(255.0)).astype(np.float16).view(np.uint16))


def test_flat_normal_map_gives_key_zeros_normal():
    """A map of (128, 128): rg * 2 - 1 = 1 / 255, not 0 - UNORM8 has no exact half -, so the normal is key 0's (0, 0, -1) tilted by
    (1, -1) / 255 along the tangent (1, 0, 0) and the bitangent cross(n, t) * w = (0, -1, 0): the hand value, and within 2^-7 of key 0's."""
    out = _run("flat_normal_map")
    a = out["A"].view(np.float16).astype(np.float64)
    e = 1.0 / 255.0
    v = np.array([e, -e, -np.sqrt(1.0 - 2 * e * e)])
    assert np.abs(a[:, :, :3] - v / np.linalg.norm(v)).max() <= 2.0 ** -11
    draws, _ = hand_cases()["flat_normal_map"]
    cam = D.hand_camera(W, H)
    depth, _ = D.depth_prepass(draws, *cam, W, H)
    plain = G.gbuffer_pass(draws, *cam, depth, W, H)
    assert np.abs(a - plain["A"].view(np.float16).astype(np.float64)).max() <= 2.0 ** -7
    for k in ("B", "C", "hdr", "keys", "object_id"):
        assert np.array_equal(out[k], plain[k])


def test_key_zero_and_missing_materials_are_section_3_9():
    w, h, seed = X.SOUPS[0]
    draws, view, proj, depth, out = soup_reference(w, h, seed)
    plain = G.gbuffer_pass(draws, view, proj, depth, w, h)
    invalid = [dict(m, **{name: X.Tex(m[name].levels, m[name].srgb, valid=False) for name, _, _ in X.MAPS}) for m in soup_materials(seed)]
    for mats in ([], [{"key": 0}] * len(draws), [dict(m, key=16) for m in soup_materials(seed)], invalid):
        got = X.gbuffer_pass(draws, view, proj, depth, w, h, materials=mats)
        for k in ("A", "B", "C", "hdr", "keys", "object_id", "stats"):
            assert np.array_equal(got[k], plain[k]), k


def _texel(rgb):
    """The fp16 bits of an unfiltered UNORM texel under an emissive factor of 1."""
    return (np.asarray(rgb, np.uint8) / np.float32(255.0)).astype(np.float16).view(np.uint16)


@pytest.mark.parametrize("name,mips", [("nan_u_one_level", 1), ("nan_u_four_levels", 4), ("inf_v", 4), ("nan_uv", 4)])
def test_non_finite_texcoord_reads_texel_zero_of_the_coarsest_level(name, mips):
    """A NaN or infinite TEXCOORD component makes both transformed coordinates non-finite - ApplyTextureTransform's rotation multiplies
    each component into both outputs, and NaN * 0 and inf * 0 are NaN - so column and row both count as 0 (rule 6): texel (0, 0), on
    every texel of the quad, not texel (0, py). The differences are NaN: N = 4 (rule 3), rho2 NaN, L = 256 (mips - 1) (rule 4, the
    exponent field 255), f = 0. The four probes coincide and the sum of four equal values divided by 4 is exact. On the one-level
    8 x 8 ramp that is R, G, B = (0, 255, 0); on the four-level one the 1 x 1 level 3: (96, 159, 0)."""
    out = _run(name)
    N, L = _info(out)
    assert N.size == 64 and (N == 4).all() and (L == 256 * (mips - 1)).all()
    want = _texel([0, 255, 0] if mips == 1 else [96, 159, 0])
    assert (out["hdr"][:, :, :3] == want).all()


def test_the_coordinate_limit_on_both_sides():
    """The 13 x 7 ramp at v = 0.5 (y = 3.0: row 3, weight 0) and a constant u: no footprint, N = 1, L = 0, x an integer (weight 0), so
    the sample is texel (x mod 13, 3), R = 16 (x mod 13) + 3, with x mod 13 from Python's integers; a dropped x is column 0."""
    us = boundary_coordinates()
    limit = 2 ** 30
    for name, u in us.items():
        out = _run(f"limit_{name}")
        N, L = _info(out)
        assert N.size == 64 and (N == 1).all() and (L == 0).all()
        x = int(np.float32(np.float32(np.float32(u) * np.float32(13.0)) - np.float32(0.5)))
        assert (abs(x) <= limit) == name.startswith("kept")
        column = x % 13 if abs(x) <= limit else 0
        r = 16 * column + 3
        assert (out["hdr"][:, :, :3] == _texel([r, 255 - r, column])).all(), name
    # the search found the limit itself: 2^30 mod 13 = 12 and -2^30 mod 13 = 1 (the kernel's r < 0; r += size at magnitude)
    assert int(np.float32(us["kept_positive"]) * np.float32(13.0)) == limit and limit % 13 == 12 and -limit % 13 == 1


@pytest.mark.parametrize("name", ["huge_gradient", "huge_gradient_past_limit"])
def test_huge_finite_derivatives_take_the_exponent_path_to_the_coarsest_level(name):
    """u = 2^26 px, v = 2^26 py on the four-level 8 x 8 ramp: P = 2^29 texels, rho2 about 2^58 - finite, so the level comes from the
    exponent (128 (e - 127) clamped), not from the special case - L = 768. Level 3 is 1 x 1: (96, 159, 0) whatever the coordinate, kept
    (2^26: u <= 2^29 stays within 2^30 texels of one) or dropped (2^28: u > 2^30 from the fifth column and row on)."""
    out = _run(name)
    N, L = _info(out)
    rows, _, _, _, coords = out["shade32"]["info"]["emissive"][0]
    assert N.size == 64 and (L == 768).all() and np.isfinite(coords).all()
    d = np.abs(coords[:, 2:] - coords[:, [0, 1, 0, 1]]).max()
    assert 2.0 ** 25 <= d <= 2.0 ** 29  # the quad's differences: finite and huge
    assert (np.abs(coords[:, :2]).max() > 2.0 ** 30) == (name == "huge_gradient_past_limit")
    assert (out["hdr"][:, :, :3] == _texel([96, 159, 0])).all()


@pytest.mark.parametrize("mips", CHAIN_MIPS)
def test_long_chain_nan_reads_the_last_level(mips):
    """NaN TEXCOORD on a chain of `mips` levels: d = mips - 1, f = 0: that level's one texel."""
    out = _run(f"chain{mips}_nan")
    N, L = _info(out)
    assert N.size == 64 and (N == 4).all() and (L >> 8 == mips - 1).all() and (L & 255 == 0).all()
    assert (out["hdr"][:, :, :3] == _texel(chain_texture(mips).levels[mips - 1][0, 0, :3])).all()


@pytest.mark.parametrize("mips,g,d", CHAIN_GRADIENTS)
def test_long_chain_gradient_blends_levels_past_the_chain(mips, g, d):
    """A finite gradient (see CHAIN_GRADIENTS): the level d it reaches, with a fraction where the chain goes on behind it (two 1 x 1
    levels past the end of the chain blended, lo + f (hi - lo)) and f = 0 where d is the clamp mips - 1."""
    out = _run(f"chain{mips}_gradient_2p{int(np.log2(g))}")
    N, L = _info(out)
    want_l = min(int(np.floor(256 * (np.log2(g) + np.log2(6.0)))), 256 * (mips - 1))
    assert N.size == 64 and (N == 2).all() and (L >> 8 == d).all() and (np.abs(L - want_l) <= (0 if d == mips - 1 else 1)).all()
    levels = chain_texture(mips).levels
    lo = levels[d][0, 0, :3] / 255.0
    if d == mips - 1:
        assert (L & 255 == 0).all()
        assert (out["hdr"][:, :, :3] == _texel(levels[d][0, 0, :3])).all()
    else:
        assert d >= 32 and (L & 255 != 0).all()
        f = ((L & 255) / 256.0).reshape(8, 8, 1)
        want = lo + f * (levels[d + 1][0, 0, :3] / 255.0 - lo)
        assert np.abs(_emissive(out) - want).max() <= 2.0 ** -11  # fp16 rounding of a value below 1


def test_host_tables():
    dec, lod = X.tables()
    assert dec.dtype == np.float32 and dec.shape == (256,) and lod.dtype == np.float32 and lod.shape == (127,)
    assert np.array_equal(dec, G.srgb_decode(np.arange(256)).astype(np.float32)) and dec[0] == 0 and dec[255] == 1
    ref = X.lod_reference()
    assert (np.abs(lod.astype(np.float64) - ref) <= np.spacing(ref.astype(np.float32)) / 2).all() and (np.diff(lod) > 0).all()
    assert 1 < lod[0] and lod[-1] < 2 and lod[63] == np.float32(np.sqrt(2.0))


def test_level_of_detail_against_float64():
    """L over a sweep of rho^2 (every exponent of the range a 65535-texel texture can reach, random mantissas, and the thresholds'
    neighbours) against floor(128 log2 rho^2) in float64. The two differ only where rho^2 lies within the fp32 rounding of a threshold:
    a table entry is 2^(j / 128) rounded to fp32, so a mantissa between the entry and the irrational value falls on the other side."""
    rng = np.random.default_rng(5)
    e = rng.integers(-20, 34, 200000)
    m = rng.uniform(1.0, 2.0, 200000).astype(np.float32)
    _, lod = X.tables()
    near = np.concatenate([np.nextafter(lod, np.float32(0)), lod, np.nextafter(lod, np.float32(4))])
    rho2 = np.concatenate([np.ldexp(m, e), np.ldexp(near, 3), np.float32([1.0, 4.0, 2.0 ** -126, 0.0])]).astype(np.float32)
    L = X.level_of_detail(rho2, 17)
    L64 = X.level_of_detail64(rho2.astype(np.float64), 17)
    differ = L != L64
    print(f"L differs from floor(256 log2 rho) on {int(differ.sum())} of {rho2.size} values")
    assert differ.sum() <= 127 and (np.abs(L - L64)[differ] == 1).all()
    mant = np.ldexp(rho2[differ].astype(np.float64), -np.floor(np.log2(rho2[differ].astype(np.float64))).astype(int))
    ref = X.lod_reference()
    assert all(np.abs(ref - v).min() <= 2.0 ** -23 for v in mant)  # each within an fp32 ulp of a threshold
    assert X.level_of_detail(np.float32([np.inf, np.nan, 0.0, 1e-45, 1e30]), 5).tolist() == [1024, 1024, 0, 0, 1024]


_SOUP = {}


def soup_materials(seed):
    return X.soup_materials(seed)


def soup_reference(w, h, seed):
    """(draws, view, projection, depth, precise textured result) of a soup, computed once and left unchanged."""
    key = (w, h, seed)
    if key not in _SOUP:
        draws = X.soup(w, h, seed)
        view, proj = D.soup_camera(w, h)
        depth, _ = D.depth_prepass(draws, view, proj, w, h)
        out = X.gbuffer_pass(draws, view, proj, depth, w, h, materials=X.soup_materials(seed), precise=True)
        for v in out.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        depth.setflags(write=False)
        _SOUP[key] = (draws, view, proj, depth, out)
    return _SOUP[key]


@pytest.mark.parametrize("w,h,seed", X.SOUPS)
def test_soup_conditions(w, h, seed):
    """What the GPU test's byte equality is worth."""
    draws, view, proj, depth, out = soup_reference(w, h, seed)
    g, r = out["gather"], out["shade32"]
    bits = r["bits"]
    assert set(bits.tolist()) == set(range(16))  # every key
    N = np.concatenate([n for runs in r["info"].values() for (_, n, _, _, _) in runs])
    L = np.concatenate([l for runs in r["info"].values() for (_, _, l, _, _) in runs])
    for n in (1, 2, 3, 4):
        assert (N == n).mean() >= 0.01, n
    mats = X.soup_materials(seed)
    top = [(l == 256 * (len(mats[int(g["slot"][rows[0]])][name].levels) - 1)).any() for name, runs in r["info"].items() for (rows, _, l, _, _) in runs
           if len(mats[int(g["slot"][rows[0]])][name].levels) > 1]
    assert (L == 0).any() and any(top) and ((L & 255) != 0).mean() >= 0.01  # both clamps and interior fractions
    assert (g["second"] & (bits != 0)).sum() >= 10  # a near-cut triangle's second piece is textured
    # partners: the horizontal or vertical partner's edge values say it lies outside the triangle; a partner column / row outside the target
    step_x = np.where(g["px"] & 1, -256, 256)[:, None]
    outside_triangle = ((g["lam"] + step_x * g["dsx"]) < 0).any(axis=1) & (bits != 0)
    px_partner, py_partner = g["px"] ^ 1, g["py"] ^ 1
    outside_target = ((px_partner >= w) | (py_partner >= h)) & (bits != 0)
    assert outside_triangle.any() and (outside_target.any() or w % 2 == 0)
    if w % 2:
        assert outside_target.any()


# The row-band splits of tests/test_gpu_gbuffer_band_frame.py on the 257 x 130 soup: (row0, rows) per band
BAND_SPLITS = {"2 x 65": [(0, 65), (65, 65)], "5 x 26": [(26 * k, 26) for k in range(5)], "unequal": [(0, 37), (37, 41), (78, 52)]}


def test_band_seam_conditions():
    """What the band frames' byte equality with the whole frame is worth: at every seam triangles win texels on both sides, one of
    them a triangle the raster serves from the large-triangle queue (its won texels alone lie in more than 64 8 x 8 stamps, so its
    bounding box does); at the odd seam (rows 64 | 65) both rows hold textured texels, each one's vertical quad partner (row y ^ 1)
    in the other band; below every first band lies a textured second piece of a near-cut triangle."""
    w, h, seed = X.SOUPS[1]
    out = soup_reference(w, h, seed)[4]
    g, bits, keys = out["gather"], out["shade32"]["bits"], out["keys"]
    stamp = (np.arange(h)[:, None] >> 3) * 64 + (np.arange(w)[None, :] >> 3)
    for name, split in BAND_SPLITS.items():
        assert sum(rows for _, rows in split) == h and all(a + n == b for (a, n), (b, _) in zip(split, split[1:]))
        for seam, _ in split[1:]:
            both = (set(keys[seam - 1].tolist()) & set(keys[seam].tolist())) - {0}
            assert len(both) >= 4, (name, seam)
            large = [k for k in both if np.unique(stamp[keys == k]).size > 64]
            assert large, (name, seam)
        assert (g["second"] & (bits != 0) & (g["py"] >= split[1][0])).any(), name
    for row in (64, 65):
        assert ((g["py"] == row) & (bits != 0)).sum() >= 20, row
    assert 64 ^ 1 == 65


def edge_soup_reference():
    """(draws, view, projection, depth, materials, fp32 textured result) of the 64 x 64 soup under soup_materials(seed, shapes=EDGE_SHAPES),
    computed once and left unchanged. The soup's own triangles reach every condition below: none were added."""
    if "edge" not in _SOUP:
        w, h, seed = X.SOUPS[0]
        draws, view, proj, depth, _ = soup_reference(w, h, seed)
        mats = X.soup_materials(seed, shapes=X.EDGE_SHAPES)
        out = X.gbuffer_pass(draws, view, proj, depth, w, h, materials=mats)
        for v in out.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _SOUP["edge"] = (draws, view, proj, depth, mats, out)
    return _SOUP["edge"]


def test_edge_shape_soup_conditions():
    """What the GPU test's byte equality is worth on textures at the ends of ur_texture2d's ranges."""
    draws, view, proj, depth, mats, out = edge_soup_reference()
    g, r = out["gather"], out["shade32"]
    assert set(r["bits"].tolist()) == set(range(16))
    shapes, counts, seam, last_of_tall = set(), np.zeros(5, np.int64), 0, 0
    bottom = top = fractions = 0
    for name, runs in r["info"].items():
        for rows, N, L, taps, _ in runs:
            tex = mats[int(g["slot"][rows[0]])][name]
            mips = len(tex.levels)
            shapes.add((tex.width, tex.height, mips))
            counts += np.bincount(N, minlength=5)
            bottom, top, fractions = bottom + int((L == 0).sum()), top + int((L == 256 * (mips - 1)).sum() if mips > 1 else 0), fractions + int(((L & 255) != 0).sum())
            if tex.width == 65535:  # level 0 taps of a used probe whose first column is the last one: the second is column 0
                used = np.arange(4)[None, :] < N[:, None]
                seam += int((used & ((L >> 8) == 0)[:, None] & (np.mod(taps[:, :, 0, 0], 65535) == 65534)).any(axis=1).sum())
            if (tex.width, tex.height, mips) == (1, 65535, 16):
                last_of_tall += int(((L >> 8) == 15).sum())
    assert shapes == set(X.EDGE_SHAPES)
    assert (counts[1:] >= 40).all(), counts  # every probe count, on 1 % of the target's texels each
    assert bottom and top and fractions >= 40
    assert seam >= 1 and last_of_tall >= 1


def test_accuracy_over_the_soups():
    worst_a, worst_c = 0.0, 0
    for w, h, seed in X.SOUPS:
        left_out, a, c = X.accuracy(soup_reference(w, h, seed)[4])
        print(f"{w} x {h}: {100 * left_out:.3f} % left out, A max error {a:.4f} fp16 ulps of the float64 value, C max code difference {c}")
        assert left_out <= 0.02
        worst_a, worst_c = max(worst_a, a), max(worst_c, c)
    assert worst_a <= X.A_ULPS_BOUND and worst_c <= X.C_CODES_BOUND
    assert abs(worst_a - X.MEASURED_A_ULPS) <= 0.01 * X.MEASURED_A_ULPS and worst_c == X.MEASURED_C_CODES, "the documented maxima are not the measured ones"
    assert X.A_ULPS_BOUND == G.bound(X.MEASURED_A_ULPS) and X.C_CODES_BOUND == G.bound(X.MEASURED_C_CODES)
