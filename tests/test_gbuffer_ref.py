"""The GBuffer rule as tests/gbuffer_ref.py restates it: answers worked out by hand on an 8 x 8 target under
depth_ref.hand_camera, the sRGB threshold table, the key split, and the accuracy of the fp32 resolve against float64 over the soups of
the GPU test."""
import numpy as np
import pytest

from tests import depth_ref as D
from tests import gbuffer_ref as G
from tests.test_depth_ref import CORNER, ONE_OUT

W = H = 8
HALF_ONE = 0x3C00


def _draw(tris, clip=False, normals=None, colors=None, **kw):
    """tris as tests/test_depth_ref.py gives them: target position and view depth per vertex, or (clip=True) clip (cx, cy, cw)."""
    pos = np.array([v if clip else D.at(*v, W, H) for t in tris for v in t], np.float32)
    return G.GDraw(G.vertex_buffer(pos, normals, colors), np.arange(pos.shape[0], dtype=np.uint32), **kw)


def _run(draws, flags=0, **kw):
    cam = D.hand_camera(W, H)
    depth, _ = D.depth_prepass(draws, *cam, W, H, flags=flags)
    return G.gbuffer_pass(draws, *cam, depth, W, H, flags=flags, **kw), depth


def _half(*v):
    return np.array(v, np.float32).astype(np.float16).view(np.uint16).tolist()


def hand_cases():
    """name -> draws; the GPU test runs them too."""
    quad = [((0, 0, 0.25), (0, 8, 0.25), (8, 0, 0.25)), ((8, 0, 0.25), (0, 8, 0.25), (8, 8, 0.25))]
    near = [tuple((x, y, 0.1875) for x, y, _ in CORNER)]
    return {
        "corner": [_draw([CORNER], base_color=np.float32([0.5, 0.25, 1.0]), emissive=np.float32([1, 2, 3]), metallic=0.5, roughness=0.25, object_id=77)],
        "one_vertex_behind": [_draw([ONE_OUT], clip=True, colors=[[1, 0, 0], [0, 1, 0], [0, 0, 1]], object_id=5)],
        "same_quad_twice": [_draw(quad, base_color=np.float32([1, 0, 0]), object_id=1), _draw(quad, base_color=np.float32([0, 1, 0]), object_id=2)],
        "nearer_earlier_keeps": [_draw(near, base_color=np.float32([1, 0, 0]), object_id=1), _draw(quad, base_color=np.float32([0, 1, 0]), object_id=2)],
        "zero_normal": [_draw([CORNER], normals=np.zeros((3, 3), np.float32), object_id=9)],
    }


def test_tie_triangle():
    """Section 3.8's tie triangle: the 28 centres with px + py <= 6 carry the key (1 << 31) | 0 (one command: T = 31); the normal (0, 0, -1)
    under the identity view stays, the view depth is -1/4, the albedo BaseColor * 1; everything else holds the clear values."""
    out, _ = _run(hand_cases()["corner"])
    inside = np.array([[x + y <= 6 for x in range(W)] for y in range(H)])
    assert G.key_bits(1) == 31 and np.array_equal(out["keys"], np.where(inside, np.uint32(1 << 31), np.uint32(0)))
    assert out["stats"].tolist() == [1, 0, 0, 0, 0, 0]
    assert (out["A"][inside] == _half(0, 0, -1, -0.25)).all() and (out["A"][~inside] == [0, 0, 0, HALF_ONE]).all()
    assert (out["B"][inside] == _half(0.04, 0.5, 0.25, 1)).all() and (out["B"][~inside] == [0, 0, 0, HALF_ONE]).all()
    assert (out["hdr"][inside] == _half(1, 2, 3, 1)).all() and (out["hdr"][~inside] == [0, 0, 0, HALF_ONE]).all()
    codes = [int(G.srgb_encode(np.float32(v))) for v in (0.5, 0.25, 1.0)]
    assert codes == [188, 137, 255]  # round(255 * srgb(x))
    assert (out["C"][inside] == (codes[0] | codes[1] << 8 | codes[2] << 16 | 0xFF000000)).all() and (out["C"][~inside] == 0xFF000000).all()
    assert (out["object_id"][inside] == 77).all() and (out["object_id"][~inside] == 0).all()


def test_one_vertex_behind_the_near_plane_pieces_agree():
    """Section 3.8's cut triangle: a (0,0), b (0,8) at w = 1/4, c behind; pieces (a, b, p) - 12 centres - and (a, p, q) - 10 centres -
    carry ONE key. Target depth is 1/2 + X / 8 in both, so clip w = (1/8) / depth and the view depth -w is one function of X across the
    diagonal a-p; the colour weights are (1 - t) at the originals and t at c with t = 2 (1 - w / (1/4)) by the same function: the blue
    share of c is t / 2 ... the two pieces' texels on either side of the diagonal follow the same formula."""
    out, depth = _run(hand_cases()["one_vertex_behind"])
    first = {(x, y) for x in range(8) for y in range(8) if x < y and x + y <= 6}
    second = {(x, y) for x in range(4) for y in range(x + 1)}
    covered = {(int(x), int(y)) for y, x in np.argwhere(out["keys"] != 0)}
    assert covered == first | second and out["stats"].tolist() == [2, 0, 0, 0, 1, 0]
    assert (out["keys"][out["keys"] != 0] == np.uint32(1 << 31)).all()
    a = out["A"].view(np.float16).astype(np.float64)
    c = out["C"]
    for x, y in first | second:
        w_clip = 0.125 / (0.5 + (x + 0.5) / 8)  # exact in float64
        assert abs(a[y, x, 3] + w_clip) <= 2.0 ** -13, (x, y)  # 1 fp16 ulp of a value in [1/8, 1/4)
        # c = (1/4, 1/4, w 0): along any line of the triangle w falls linearly in clip space from 1/4 to 0, so c's share is 1 - 4 w
        blue = 1.0 - 4.0 * w_clip
        assert abs(int(c[y, x] >> 16 & 0xFF) - int(G.srgb_encode(np.float32(blue)))) <= 1, (x, y)
    # the diagonal's two sides: texel (x, x) is the second piece's, (x, x + 1) the first's - the same X, so the same depth and blue
    for x in range(3):
        assert a[x, x, 3] == a[x + 1, x, 3] and (c[x, x] >> 16) == (c[x + 1, x] >> 16)


def test_equal_depth_goes_to_the_later_command_and_a_nearer_earlier_one_keeps_its_texels():
    out, _ = _run(hand_cases()["same_quad_twice"])
    T = G.key_bits(2)
    assert T == 30 and (out["keys"] >> T == 2).all() and (out["object_id"] == 2).all()
    assert (out["C"] == (0 | 255 << 8 | 0 | 0xFF000000)).all()
    # within the later command the quad's diagonal texels belong to exactly one triangle each (the top-left rule)
    assert set((out["keys"] & ((1 << T) - 1)).reshape(-1).tolist()) == {0, 1}
    out, depth = _run(hand_cases()["nearer_earlier_keeps"])
    inside = np.array([[x + y <= 6 for x in range(W)] for y in range(H)])
    assert (out["object_id"][inside] == 1).all() and (out["object_id"][~inside] == 2).all()
    assert (depth[inside] == np.float32(0.125) / np.float32(0.1875)).all()
    # against another depth the picture is still defined: with depth = 0 every fragment passes and the later command takes every texel
    cam = D.hand_camera(W, H)
    late = G.gbuffer_pass(hand_cases()["nearer_earlier_keeps"], *cam, np.zeros((H, W), np.float32), W, H)
    assert (late["object_id"] == 2).all()
    none = G.gbuffer_pass(hand_cases()["nearer_earlier_keeps"], *cam, np.full((H, W), 2.0, np.float32), W, H)
    assert not none["keys"].any() and (none["C"] == 0xFF000000).all()


def test_zero_normal_gives_nan_and_d24_changes_nothing_but_the_test():
    out, _ = _run(hand_cases()["zero_normal"])
    inside = out["keys"] != 0
    a = out["A"].view(np.float16)
    assert inside.sum() == 28 and np.isnan(a[inside][:, :3]).all() and (a[inside][:, 3] == np.float16(-0.25)).all()
    for name, draws in hand_cases().items():
        plain, _ = _run(draws)
        d24, _ = _run(draws, flags=G.QUANTIZE_D24)
        for k in ("keys", "B", "C", "hdr", "object_id", "stats"):
            assert np.array_equal(plain[k], d24[k]), (name, k)


def test_threshold_table():
    tab = G.table()
    ref = G.srgb_encode_reference()
    assert tab.dtype == np.float32 and tab.shape == (255,) and (np.diff(tab) > 0).all()
    ulp = np.spacing(ref.astype(np.float32)).astype(np.float64)
    assert (np.abs(tab.astype(np.float64) - ref) <= ulp).all()
    codes = np.arange(256)
    assert np.array_equal(G.srgb_encode(G.srgb_decode(codes).astype(np.float32)), codes.astype(np.uint32))
    assert int(G.srgb_encode(np.float32(np.nan))) == 0 and int(G.srgb_encode(np.float32(-1.0))) == 0
    assert int(G.srgb_encode(np.float32(np.inf))) == 255 and int(G.srgb_encode(np.float32(7.0))) == 255


@pytest.mark.parametrize("count,bits", [(1, 31), (2, 30), (3, 30), (4, 29), (5, 29), (255, 24), (256, 23), (65535, 16), (2 ** 24 - 1, 8)])
def test_key_split(count, bits):
    assert G.key_bits(count) == bits
    assert (count << bits) < 2 ** 32  # the last ordinal + 1 fits
    assert G.key_bits(count, 4) == 4


_SOUP = {}


def soup_reference(w, h, seed):
    """(draws, view, projection, depth, precise result) of a soup, computed once and left unchanged."""
    key = (w, h, seed)
    if key not in _SOUP:
        draws = G.soup(w, h, seed)
        view, proj = D.soup_camera(w, h)
        depth, _ = D.depth_prepass(draws, view, proj, w, h)
        out = G.gbuffer_pass(draws, view, proj, depth, w, h, precise=True)
        for v in out.values():
            v.setflags(write=False)
        depth.setflags(write=False)
        _SOUP[key] = (draws, view, proj, depth, out)
    return _SOUP[key]


@pytest.mark.parametrize("w,h,seed", G.SOUPS)
def test_soup_conditions(w, h, seed):
    """What the GPU test's byte equality is worth: cut triangles resolve, ties exist, the stride-12 command is counted, the weights agree
    with the polygon depth_ref cuts."""
    draws, view, proj, depth, out = soup_reference(w, h, seed)
    s = out["stats"]
    assert s[0] > 300 and s[4] >= 100 and s[5] >= 20 and s[1] == draws[3].count() // 3 and draws[3].stride == 12
    assert (out["keys"] != 0).mean() >= 0.25
    T = G.key_bits(len(draws))
    assert set((out["keys"][out["keys"] != 0] >> T).tolist()) == {1, 3, 5}  # draws 0, 2 and 4: 1 has InstanceCount 0, 3 is unsupported


def test_accuracy_over_the_soups():
    worst_a, worst_c = 0.0, 0
    for w, h, seed in G.SOUPS:
        a, c = G.accuracy(soup_reference(w, h, seed)[4])
        print(f"{w} x {h}: A max error {a:.4f} fp16 ulps of the float64 value, C max code difference {c}")
        worst_a, worst_c = max(worst_a, a), max(worst_c, c)
    assert worst_a <= G.A_ULPS_BOUND and worst_c <= G.C_CODES_BOUND
    assert abs(worst_a - G.MEASURED_A_ULPS) <= 0.01 * G.MEASURED_A_ULPS and worst_c == G.MEASURED_C_CODES, "the documented maxima are not the measured ones"
    assert G.A_ULPS_BOUND == G.bound(G.MEASURED_A_ULPS) and G.C_CODES_BOUND == G.bound(G.MEASURED_C_CODES)
