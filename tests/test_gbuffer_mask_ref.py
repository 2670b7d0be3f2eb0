"""The alpha-masked GBuffer rule as tests/gbuffer_mask_ref.py restates it: answers worked out by hand on an 8 x 8
target under depth_ref.hand_camera (power-of-two geometry: every weight, and so every alpha, is exact), the soups' coverage conditions
and the accuracy of the fp32 rule against float64."""
import numpy as np
import pytest

from tests import depth_ref as D
from tests import gbuffer_mask_ref as M
from tests import gbuffer_ref as G
from tests import gbuffer_tex_ref as X
from tests.test_depth_ref import ONE_OUT

W = H = 8
MASK, MAP = M.ALPHA_MASK, X.BASE_COLOR


def quad(z, alpha_of=lambda x, y: 1.0, **kw):
    """The screen-filling quad at view depth z (target depth 1 / (8 z)), TEXCOORD (X / 8, Y / 8) - one texel of an 8 x 8 texture per pixel,
    centres on centres - and COLOR.a = alpha_of(X, Y) at the corner (X, Y)."""
    corners = [(0, 0), (0, 8), (8, 0), (8, 0), (0, 8), (8, 8)]
    v = np.zeros((6, 16), np.float32)
    for k, (x, y) in enumerate(corners):
        v[k, 0:3] = D.at(x, y, z, W, H)
        v[k, 3:6] = (0, 0, -1)
        v[k, 6:8] = (x / 8.0, y / 8.0)
        v[k, 8:12] = (1, 0, 0, 1)
        v[k, 12:15] = 1.0
        v[k, 15] = alpha_of(x, y)
    return M.MaskDraw(v.reshape(-1).view(np.uint8).copy(), np.arange(6, dtype=np.uint32), **kw)


def texture(alpha):
    """An 8 x 8 one-level texture whose texel (x, y) has A = alpha[y, x] and R = G = B = 255."""
    t = np.full((8, 8, 4), 255, np.uint8)
    t[:, :, 3] = alpha
    return X.Tex([t], True)


def holes(*at):
    a = np.full((8, 8), 255, np.uint8)
    for x, y in at:
        a[y, x] = 0
    return a


CHECKER = np.fromfunction(lambda y, x: np.where((x + y) % 2 == 0, 255, 0), (8, 8)).astype(np.uint8)
STRADDLER_ALPHA, STRADDLER_CUTOFF = (1.0, 0.0, 0.5), 0.46875


def hand_cases():
    """name -> (draws, materials, opaque slots, masked slots); the GPU test runs them too."""
    nan = float("nan")
    solid = {"key": MASK | MAP, "base_color": texture(holes())}
    pos = np.array(ONE_OUT, np.float32)
    v = np.zeros((3, 16), np.float32)
    v[:, 0:3], v[:, 3:6], v[:, 8:12], v[:, 12:15], v[:, 15] = pos, (0, 0, -1), (1, 0, 0, 1), 1.0, STRADDLER_ALPHA
    straddler = M.MaskDraw(v.reshape(-1).view(np.uint8).copy(), np.arange(3, dtype=np.uint32), cutoff=STRADDLER_CUTOFF)
    return {
        "checkerboard": ([quad(0.25)], [{"key": MASK | MAP, "base_color": texture(CHECKER)}], [], [0]),
        "color_ramp": ([quad(0.25, lambda x, y: x / 8.0, cutoff=4.5 / 8.0)], [{"key": MASK}], [], [0]),
        "alpha_equals_cutoff": ([quad(0.5, alpha=0.5, cutoff=0.5), quad(0.25, alpha=0.5, cutoff=float(np.nextafter(np.float32(0.5), np.float32(1))))],
                                [{"key": MASK}, {"key": MASK}], [], [0, 1]),
        "nan_cutoff": ([quad(0.5, alpha=0.0, cutoff=nan), quad(0.25, alpha=0.0, cutoff=0.5)], [{"key": MASK}, {"key": MASK}], [], [0, 1]),
        "nan_alpha": ([quad(0.5, lambda x, y: nan if (x, y) == (8, 8) else 0.0, cutoff=0.5)], [{"key": MASK}], [], [0]),
        "bit4_clear": ([quad(0.5, base_color=np.float32([1, 0, 0])), quad(0.25, alpha=0.0, base_color=np.float32([0, 1, 0]))],
                       [{"key": 0}, {"key": MAP, "base_color": texture(CHECKER)}], [0], [1]),
        "three_layers": ([quad(1.0, base_color=np.float32([1, 0, 0])), quad(0.5, base_color=np.float32([0, 1, 0])), quad(0.25, base_color=np.float32([0, 0, 1]))],
                         [solid, {"key": MASK | MAP, "base_color": texture(holes((3, 4), (2, 2)))}, {"key": MASK | MAP, "base_color": texture(holes((3, 4), (6, 1)))}],
                         [], [0, 1, 2]),
        "equal_depth_masked_later": ([quad(0.5, base_color=np.float32([1, 0, 0])), quad(0.5, base_color=np.float32([0, 1, 0]))], [{"key": 0}, solid], [0], [1]),
        "equal_depth_masked_earlier": ([quad(0.5, base_color=np.float32([1, 0, 0])), quad(0.5, base_color=np.float32([0, 1, 0]))], [solid, {"key": 0}], [1], [0]),
        "behind_opaque": ([quad(0.5), quad(1.0)], [{"key": 0}, solid], [0], [1]),
        "near_straddler": ([straddler], [{"key": MASK}], [], [0]),
    }


def run_case(case, flags=0, precise=False):
    draws, mats, opaque, masked = case
    cam = D.hand_camera(W, H)
    depth, _ = D.depth_prepass(draws, *cam, W, H, flags=flags, slots=opaque)
    out = M.masked_pass(draws, *cam, depth, W, H, materials=mats, flags=flags, select=[(s, s) for s in opaque], mask_select=[(s, s) for s in masked], precise=precise)
    return out, depth


def _key(slot, count, tri=None):
    T = G.key_bits(count)
    return (slot + 1) << T if tri is None else ((slot + 1) << T) | tri


def test_checkerboard_keeps_exactly_the_opaque_texels():
    """A = 255 where x + y is even, 0 elsewhere, one texel per pixel (N = 1, L = 0: the sample is the texel): alpha 1 or 0 against 0.5."""
    out, depth = run_case(hand_cases()["checkerboard"])
    even = np.fromfunction(lambda y, x: (x + y) % 2 == 0, (8, 8))
    assert not depth.any()
    assert np.array_equal(out["keys"] != 0, even) and out["won"] == 32
    assert np.array_equal(out["depth"], np.where(even, np.float32(0.5), np.float32(0)))
    assert np.array_equal(out["keys64"] != 0, even) and (out["keys64"][even] >> np.uint64(32) == 0x3F000000).all()
    layer = out["layers"][0]
    assert (layer["N"] == 1).all() and layer["sampled"].all() and set(layer["alpha"].tolist()) == {0.0, 1.0}
    assert (out["C"][~even] == 0xFF000000).all() and (out["C"][even] == 0xFFFFFFFF).all()
    assert out["mask_stats"].tolist() == [2, 0, 0, 0, 0, 0] and out["stats"].tolist() == [0] * 6


def test_color_ramp_crosses_the_cutoff_without_a_texture():
    """COLOR.a = X / 8 at the corners: alpha = (px + 0.5) / 8 exactly; the cutoff 4.5 / 8 keeps px = 4 (equal) and everything right of it."""
    out, _ = run_case(hand_cases()["color_ramp"])
    assert np.array_equal(out["layers"][0]["alpha"].reshape(8, 8), np.tile((np.arange(8, dtype=np.float32) + 0.5) / 8, (8, 1)))
    assert np.array_equal(out["keys"] != 0, np.tile(np.arange(8) >= 4, (8, 1))) and out["won"] == 32
    assert not out["layers"][0]["sampled"].any()


def test_alpha_equal_to_the_cutoff_is_kept_and_a_nan_cutoff_keeps():
    out, _ = run_case(hand_cases()["alpha_equals_cutoff"])
    assert (out["keys"] >> 30 == 1).all() and (out["depth"] == 0.25).all()  # the far quad (alpha == cutoff); the near one (cutoff one ulp up) is gone
    assert sum(int(layer["discarded"].sum()) for layer in out["layers"]) == 64
    out, _ = run_case(hand_cases()["nan_cutoff"])
    assert (out["keys"] >> 30 == 1).all() and (out["depth"] == 0.25).all()  # alpha 0 < 0.5 goes, alpha 0 against a NaN cutoff stays
    out, _ = run_case(hand_cases()["nan_alpha"])
    # COLOR.a is NaN at the corner (8, 8): 0 * NaN makes the alpha of its whole triangle NaN, which stays; the other triangle's alpha is 0
    lower = np.fromfunction(lambda y, x: x + y > 6, (8, 8))
    assert np.array_equal(out["keys"] != 0, lower) and np.isnan(out["layers"][0]["alpha"].reshape(8, 8)[lower]).all()


def test_bit4_clear_discards_nothing_and_equals_the_union():
    """The masked selection's slot has key 4 (a base-colour map full of holes, COLOR.a 0, no bit 4): nothing is discarded, the nearest
    fragment wins, and keys, targets and depth are those of DepthPrepass + ur_gbuffer_pass_materials over both draws."""
    case = hand_cases()["bit4_clear"]
    out, _ = run_case(case)
    cam = D.hand_camera(W, H)
    union_depth, _ = D.depth_prepass(case[0], *cam, W, H)
    union = X.gbuffer_pass(case[0], *cam, union_depth, W, H, materials=case[1])
    for k in ("keys", "A", "B", "C", "hdr"):
        assert np.array_equal(out[k], union[k]), k
    assert np.array_equal(out["depth"], union_depth) and out["won"] == 64
    assert not any(layer["discarded"].any() for layer in out["layers"])


def test_three_layers_with_the_front_two_clipped():
    out, _ = run_case(hand_cases()["three_layers"])
    want = np.full((8, 8), 3, np.uint32)
    want[4, 3], want[1, 6] = 1, 2  # both clipped: the back layer; the front one clipped: the middle one; (2, 2) is a hole of the hidden middle layer only
    assert np.array_equal(out["keys"] >> 30, want)
    assert np.array_equal(out["depth"], np.float32(0.125) * np.float32([0, 1, 2, 4])[want])
    assert out["clipped_in_front"][4, 3] == 2 and out["clipped_in_front"][1, 6] == 1 and out["clipped_in_front"].sum() == 3 and out["won"] == 64
    blue, green, red = 0xFFFF0000, 0xFF00FF00, 0xFF0000FF
    assert out["C"][4, 3] == red and out["C"][1, 6] == green and out["C"][2, 2] == blue


def test_equal_depth_goes_to_the_larger_key_in_both_slot_orders():
    later, depth = run_case(hand_cases()["equal_depth_masked_later"])
    assert (later["keys"] >> 30 == 2).all() and later["won"] == 64 and np.array_equal(later["depth"], depth) and (depth == 0.25).all()
    earlier, depth = run_case(hand_cases()["equal_depth_masked_earlier"])
    assert (earlier["keys"] >> 30 == 2).all() and earlier["won"] == 0 and np.array_equal(earlier["depth"], depth) and not earlier["keys64"].any()
    assert (later["C"] == 0xFF00FF00).all() and (earlier["C"] == 0xFF00FF00).all()  # the later slot's colour either way


def test_masked_draw_behind_opaque_geometry_never_wins():
    out, depth = run_case(hand_cases()["behind_opaque"])
    assert (out["keys"] >> 30 == 1).all() and out["won"] == 0 and np.array_equal(out["depth"], depth) and not out["keys64"].any()
    assert out["mask_stats"].tolist() == [2, 0, 0, 0, 0, 0] and not out["layers"]


def test_near_plane_straddler_with_a_hole_across_the_cut():
    """Section 3.8's cut triangle (a, b in front, c behind: two pieces under ONE key) with COLOR.a (1, 0, 1/2) and a cutoff that runs a
    hole across the diagonal between the pieces. The survivors are those of the uncut triangle: alpha interpolated in clip space over
    the original three vertices, in float64, with no clip anywhere; no centre lies within 1/64 of the cutoff."""
    out, _ = run_case(hand_cases()["near_straddler"])
    Mx = np.array(ONE_OUT, np.float64)  # rows (cx, cy, cw)
    want = np.zeros((8, 8), bool)
    margin = 1.0
    for py in range(8):
        for px in range(8):
            ndc = np.array([(px + 0.5) / 4.0 - 1.0, 1.0 - (py + 0.5) / 4.0, 1.0])
            b = np.linalg.solve(Mx.T, ndc)
            b = b / b.sum()
            w = float(b @ Mx[:, 2])
            if (b > 1e-9).all() and w > D.NEAR:
                alpha = float(b @ np.array(STRADDLER_ALPHA))
                margin = min(margin, abs(alpha - STRADDLER_CUTOFF))
                want[py, px] = alpha >= STRADDLER_CUTOFF
    layer = out["layers"][0]
    assert layer["texel"].size == 22 and margin > 1.0 / 64
    assert np.array_equal(out["keys"] != 0, want)
    second = np.zeros(64, bool)
    # both pieces hold survivors and holes
    g = X.gather(hand_cases()["near_straddler"][0], *D.hand_camera(W, H), np.where(np.isin(np.arange(64), layer["texel"]), np.uint32(1 << 31), 0).reshape(8, 8).astype(np.uint32),
                 W, H, {0: 0}, 31)
    second[g["at"]] = g["second"]
    kept = (out["keys"] != 0).reshape(-1)
    hit = np.isin(np.arange(64), layer["texel"])
    for piece in (second, ~second):
        assert (hit & piece & kept).any() and (hit & piece & ~kept).any()
    assert out["mask_stats"].tolist() == [2, 0, 0, 0, 1, 0]


# ---- the soups ---------------------------------------------------------------------------------------------------------------------------

_SOUP = {}


def soup_reference(w, h, seed):
    """(draws, materials, opaque selection, masked selection, view, projection, depth, precise result) of a soup, computed once and left
    unchanged."""
    key = (w, h, seed)
    if key not in _SOUP:
        draws, mats = M.soup(w, h, seed), M.soup_materials(seed)
        opaque, masked = M.soup_selections()
        view, proj = D.soup_camera(w, h)
        depth, _ = D.depth_prepass(draws, view, proj, w, h, slots=[s for _, s in opaque])
        out = M.masked_pass(draws, view, proj, depth, w, h, materials=mats, select=opaque, mask_select=masked, precise=True)
        _SOUP[key] = (draws, mats, opaque, masked, view, proj, depth, out)
    return _SOUP[key]


@pytest.mark.parametrize("w,h,seed", M.SOUPS)
def test_soups_reach_what_they_are_for(w, h, seed):
    draws, mats, opaque, masked, _, _, _, out = soup_reference(w, h, seed)
    assert len(masked) * 3 == len(draws) and {mats[s]["key"] >> 4 for _, s in masked} == {0, 1} and all(mats[s]["key"] < 16 for _, s in opaque)
    assert all(0.2 < d.cutoff < 0.8 for d in draws)
    layers = out["layers"]
    n = np.concatenate([layer["N"][layer["sampled"]] for layer in layers])
    assert set(n.tolist()) == {1, 2, 3, 4}
    fragments, discarded = sum(layer["texel"].size for layer in layers), sum(int(layer["discarded"].sum()) for layer in layers)
    print(f"soup {w}x{h}: {fragments} masked fragments pass the depth test, {discarded / fragments:.1%} discarded, {len(layers)} layers, "
          f"{out['won']} texels won, {int((out['clipped_in_front'] >= 2).sum())} winners behind two or more clipped layers")
    assert 0.2 <= discarded / fragments <= 0.8
    assert (out["clipped_in_front"] >= 2).any()
    assert 0 < out["won"] < w * h and (out["opaque_keys"] != 0).any() and (out["wins"] & (out["opaque_keys"] != 0)).any()
    assert (out["depth"] >= out["depth"] * 0).all() and (out["depth"].view(np.uint32) >= _SOUP[(w, h, seed)][6].view(np.uint32)).all()


@pytest.mark.parametrize("w,h,seed", M.SOUPS)
def test_soups_accuracy_against_float64(w, h, seed):
    """float64 takes the same probes, levels, taps and discard decisions on all but a capped share of the texels; there keys and depth are
    float64's, and A and C hold section 3.10's bounds."""
    _, _, _, _, _, _, _, out = soup_reference(w, h, seed)
    resolve_differs = np.zeros(w * h, bool)
    resolve_differs[out["gather"]["at"]] = ~X.same_choices(out)
    touched = np.zeros(w * h, bool)
    for layer in out["layers"]:
        touched[layer["texel"]] = True
    touched |= out["keys"].reshape(-1) != 0
    left_out = float((out["differs"].reshape(-1) | resolve_differs).sum()) / max(int(touched.sum()), 1)
    _, a_ulps, c_codes = X.accuracy(out)
    print(f"soup {w}x{h}: {left_out:.3%} of the touched texels left out, A within {a_ulps:.2f} fp16 ulps, C within {c_codes} codes")
    assert left_out <= 0.02
    same = ~out["differs"]
    assert np.array_equal(out["keys"][same], out["keys_f64"][same]) and np.array_equal(out["depth"][same].view(np.uint32), out["depth_f64"][same].view(np.uint32))
    assert a_ulps <= X.A_ULPS_BOUND and c_codes <= X.C_CODES_BOUND
