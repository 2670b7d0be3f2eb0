"""The ObjectId rule as tests/object_id_ref.py restates it: answers worked out by hand on the 8 x 8 target of
tests/test_gbuffer_mask_ref.py (depth_ref.hand_camera: a quad at view depth z has target depth 1 / (8 z)), planted errors that each of
them must catch, and the float64 ray casters' verdict on their scenes (tests/object_id_raycast.py)."""
import numpy as np
import pytest

from tests import depth_ref as D
from tests import gbuffer_mask_ref as M
from tests import gbuffer_ref as G
from tests import object_id_raycast as OR
from tests import object_id_ref as O
from tests import raycast_ref as R
from tests import raycast_tex as T
from tests import test_gbuffer_mask_ref as TM
from tests.test_depth_ref import ONE_OUT

W = H = 8
ODD = np.fromfunction(lambda y, x: (x + y) % 2 == 1, (8, 8))  # the holes of TM.CHECKER
HALF, QUARTER = 0x3F000000, 0x3E800000                        # the bits of 0.5 and 0.25
CHECKER_MATERIAL = {"key": TM.MASK | TM.MAP, "base_color": TM.texture(TM.CHECKER)}


def _straddler(object_id):
    pos = np.array(ONE_OUT, np.float32)
    v = np.zeros((3, 16), np.float32)
    v[:, 0:3], v[:, 3:6], v[:, 8:12], v[:, 12:16] = pos, (0, 0, -1), (1, 0, 0, 1), 1.0
    return M.MaskDraw(v.reshape(-1).view(np.uint8).copy(), np.arange(3, dtype=np.uint32), object_id=object_id)


def hand_cases():
    """name -> (draws, materials, opaque slots, masked slots, depth: None = what masked_pass leaves, or a function of that depth); the GPU
    test runs them too. Every case's ObjectId selection is the union of both."""
    def raised(at, value):
        def f(depth):
            depth = depth.copy()
            depth[at[1], at[0]] = value
            return depth
        return f
    return {
        "coplanar": ([TM.quad(0.5, object_id=11), TM.quad(0.5, object_id=22)], [{"key": 0}, {"key": 0}], [0, 1], [], None),
        "depth_above": ([TM.quad(0.5, object_id=11)], [{"key": 0}], [0], [], raised((3, 2), np.float32(0.5))),
        "depth_above_corner": ([TM.quad(0.5, object_id=11)], [{"key": 0}], [0], [], raised((7, 7), np.float32(0.5))),
        "checker_later": ([TM.quad(0.5, object_id=7), TM.quad(0.25, object_id=9)], [{"key": 0}, CHECKER_MATERIAL], [0], [1], None),
        "checker_earlier": ([TM.quad(0.25, object_id=9), TM.quad(0.5, object_id=7)], [CHECKER_MATERIAL, {"key": 0}], [1], [0], None),
        "near_straddler": ([_straddler(0xC0FFEE)], [{"key": 0}], [0], [], None),
    }


def case_depth(case, flags=0):
    """The depth the case's ObjectId pass tests against: the opaque prepass raised by the masked G-buffer pass, then the case's own change."""
    draws, mats, opaque, masked, change = case
    cam = D.hand_camera(W, H)
    depth, _ = D.depth_prepass(draws, *cam, W, H, flags=flags, slots=opaque)
    if masked:
        depth = M.masked_pass(draws, *cam, depth, W, H, materials=mats, flags=flags, select=[(s, s) for s in opaque], mask_select=[(s, s) for s in masked])["depth"]
    return depth if change is None else change(depth)


def run_case(case, **wrong):
    return O.image(case[0], *D.hand_camera(W, H), case_depth(case), W, H, **wrong)


def _key(slot, count, tri=0):
    return ((slot + 1) << G.key_bits(count)) | tri


def test_coplanar_draws_at_equal_depth_go_to_the_later_slot():
    out = run_case(hand_cases()["coplanar"])
    assert (out["object_id"] == 22).all() and (out["slot"] == 1).all() and (out["depth_bits"] == QUARTER).all()
    assert set(np.unique(out["keys"]).tolist()) == {_key(1, 2, 0), _key(1, 2, 1)}  # the quad's two triangles
    assert out["stats"].tolist() == [4, 0, 0, 0, 0, 0]


def test_a_texel_whose_depth_is_above_every_fragment_stays_0():
    out = run_case(hand_cases()["depth_above"])
    rest = np.ones((8, 8), bool)
    rest[2, 3] = False
    assert out["keys"][2, 3] == 0 and out["object_id"][2, 3] == 0 and out["slot"][2, 3] == O.NO_SLOT and out["depth_bits"][2, 3] == 0
    assert (out["object_id"][rest] == 11).all() and (out["depth_bits"][rest] == QUARTER).all()
    assert O.pick(out, [(3, 2)], W, H).tolist() == [[0, 0, O.NO_SLOT, 0]]


def test_a_masked_model_drawn_later_is_picked_through_its_holes():
    """The checkerboard quad (view depth 0.25, target depth 0.5) in front of an opaque one (0.25). masked_pass leaves 0.5 where the board is
    solid and 0.25 in its holes; the board's fragment is 0.5 everywhere and passes both, alpha test or not."""
    case = hand_cases()["checker_later"]
    depth = case_depth(case)
    assert np.array_equal(depth, np.where(ODD, np.float32(0.25), np.float32(0.5)))
    out = run_case(case)
    assert (out["object_id"] == 9).all() and (out["slot"] == 1).all() and (out["depth_bits"] == HALF).all()


def test_with_the_slots_exchanged_the_opaque_model_shows_in_the_holes_only():
    out = run_case(hand_cases()["checker_earlier"])
    assert np.array_equal(out["object_id"], np.where(ODD, 7, 9)) and np.array_equal(out["slot"], np.where(ODD, 1, 0))
    assert np.array_equal(out["depth_bits"], np.where(ODD, QUARTER, HALF))  # each winner carries its own depth, not the nearest fragment's


def test_near_plane_straddler():
    """Section 3.8's cut triangle: two pieces under one key, the 22 centres tests/test_gbuffer_mask_ref.py counts, each with its own depth."""
    case = hand_cases()["near_straddler"]
    out = run_case(case)
    covered = out["keys"] != 0
    assert covered.sum() == 22 and (out["keys"][covered] == _key(0, 1, 0)).all() and (out["object_id"][covered] == 0xC0FFEE).all()
    assert np.array_equal(out["depth_bits"], case_depth(case).view(np.uint32))
    columns = np.tile(np.arange(8), (8, 1))  # the depth plane runs along x alone, across the cut: (9 + 2 px) / 16
    assert np.array_equal(out["depth_bits"].view(np.float32)[covered], ((9 + 2 * columns[covered]) / 16).astype(np.float32))
    assert out["stats"].tolist() == [2, 0, 0, 0, 1, 0]


def test_points_clamp_to_the_last_column_and_row():
    assert O.clamp_points([(W, 0xFFFFFFFF), (0xFFFFFFFF, 0), (3, 2), (7, 8)], W, H).tolist() == [[7, 7], [7, 0], [3, 2], [7, 7]]
    out = run_case(hand_cases()["depth_above_corner"])
    assert O.pick(out, [(W, 0xFFFFFFFF), (0, 0xFFFFFFFF)], W, H).tolist() == [[0, 0, O.NO_SLOT, 0], [11, int(out["keys"][7, 0]), 0, QUARTER]]


@pytest.mark.parametrize("name", sorted(hand_cases()))
def test_the_pick_is_the_image_at_every_texel(name):
    out = run_case(hand_cases()[name])
    for points in O.every_texel(W, H):
        rec = O.pick(out, points, W, H)
        for (x, y), r in zip(points, rec.tolist()):
            assert r == [int(out["object_id"][y, x]), int(out["keys"][y, x]), int(out["slot"][y, x]), int(out["depth_bits"][y, x])]
    twice = O.pick(out, [(5, 5), (1, 6), (5, 5)], W, H)
    assert twice[0].tolist() == twice[2].tolist()


# ---- planted errors: each must change a hand-worked answer ---------------------------------------------------------------------------------

def test_planted_alpha_test_fails():
    holes = lambda slot, texels: (slot == 1) & ODD.reshape(-1)[texels]  # noqa: E731  (the board's own discards)
    out = run_case(hand_cases()["checker_later"], wrong_alpha=holes)
    assert not (out["object_id"] == 9).all() and np.array_equal(out["object_id"], np.where(ODD, 7, 9))


def test_planted_nearest_fragment_fails():
    out = run_case(hand_cases()["checker_earlier"], wrong_nearest=True)
    assert not np.array_equal(out["object_id"], np.where(ODD, 7, 9)) and (out["object_id"] == 9).all()


def test_planted_greater_fails():
    out = run_case(hand_cases()["coplanar"], wrong_greater=True)
    assert not (out["object_id"] == 22).any() and not out["keys"].any()


def test_planted_unclamped_point_fails():
    out = run_case(hand_cases()["depth_above_corner"])
    right, wrong = O.pick(out, [(W, 0xFFFFFFFF)], W, H), O.pick(out, [(W, 0xFFFFFFFF)], W, H, wrong_unclamped=True)
    assert right.tolist() == [[0, 0, O.NO_SLOT, 0]] and wrong.tolist() != right.tolist() and wrong[0, 0] == 11


# ---- the soups: the image is the key raster's -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h,seed", G.SOUPS[:1])
def test_the_image_is_gbuffer_pass_keys_and_object_id(w, h, seed):
    """Under the prepass' depth and under a depth it never wrote, with and without D24: tests/gbuffer_ref.py's keys, ObjectId and stats."""
    draws = G.soup(w, h, seed)
    view, proj = D.soup_camera(w, h)
    rng = np.random.default_rng(seed)
    for flags in (0, G.QUANTIZE_D24):
        own, _ = D.depth_prepass(draws, view, proj, w, h, flags=flags)
        for depth in (own, np.where(rng.uniform(size=(h, w)) < 0.5, own, rng.uniform(0.0, 0.2, (h, w))).astype(np.float32)):
            want = G.gbuffer_pass(draws, view, proj, depth, w, h, flags=flags)
            out = O.image(draws, view, proj, depth, w, h, flags=flags)
            assert np.array_equal(out["keys"], want["keys"]) and np.array_equal(out["object_id"], want["object_id"])
            assert out["stats"].tolist() == want["stats"].tolist()
            assert ((out["depth_bits"].view(np.float32) >= depth) | (out["keys"] == 0)).all()


# ---- held independently by the ray casters --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", R.TARGETS)
@pytest.mark.parametrize("name,order", [("icosphere", (0,)), ("torus", (0,)), ("two draws", (0, 1)), ("two draws", (1, 0)), ("near-plane strip", (0, 1))])
def test_opaque_scenes_against_the_ray_caster(record_property, name, order, w, h):
    sc, rc = R.cast_scene(name, w, h)
    compared, want, left_out = OR.opaque_expectation(sc, rc)
    draws = [sc.draws[k] for k in order]
    depth, _ = D.depth_prepass(draws, sc.view, sc.proj, w, h)
    out = O.image(draws, sc.view, sc.proj, depth, w, h)
    record_property(f"{name} {order} {w}x{h}", f"left out {left_out:.2%}")
    assert left_out <= R.LEFT_OUT_CAP
    assert (compared & (want != 0)).any() and OR.held(out["object_id"], compared, want) == 0


def masked_restated(sc, w, h):
    """(the depth masked_pass leaves over the scene's own selections, the ObjectId image over all its draws against it)."""
    mats = T.ref_materials(sc.mats)
    depth, _ = D.depth_prepass(sc.draws, sc.view, sc.proj, w, h, slots=sc.opaque)
    depth = M.masked_pass(sc.draws, sc.view, sc.proj, depth, w, h, materials=mats, select=[(k, k) for k in sc.opaque], mask_select=[(k, k) for k in sc.masked])["depth"]
    return depth, O.image(sc.draws, sc.view, sc.proj, depth, w, h)


def check_masked(record_property, what, sc, rc, w, h, slot_of, got_object_id, gbuffer_keys=None):
    """The masked scene's checks, for the restatement here and the kernels in tests/test_gpu_object_id.py: the cap, the expected ids, and
    that the comparison is not vacuous."""
    compared, want, left_out, by_classify = OR.masked_expectation(sc, rc, w, h, slot_of)
    ids = {name: sc.draws[d].object_id for name, d in (("ico", 0), ("torus", 1), ("grid", 2))}
    counts = {name: int((compared & (want == i)).sum()) for name, i in ids.items()}
    text = f"{what}: {int(by_classify.sum())} texels by classify, {int((by_classify & ~compared).sum())} more left out, {left_out:.2%} left out; {counts}"
    record_property(what, text)
    print(text)
    assert left_out <= R.LEFT_OUT_CAP
    assert OR.held(got_object_id, compared, want) == 0, text
    return compared, want, counts, ids


@pytest.mark.parametrize("w,h", R.TARGETS)
@pytest.mark.parametrize("order_name", sorted(OR.MASKED_ORDERS))
def test_masked_scene_against_the_ray_caster(record_property, order_name, w, h):
    sc, rc = T.cast_scene("masked", w, h)
    moved, slot_of = OR.reordered(sc, OR.MASKED_ORDERS[order_name])
    _, out = masked_restated(moved, w, h)
    compared, want, counts, ids = check_masked(record_property, f"object_id_ref, masked ({order_name}) {w}x{h}", sc, rc, w, h, slot_of, out["object_id"])
    if order_name == "ico, torus, grid":
        # the grid is drawn last and spans the view: its id on every compared texel, which alone shows that the alpha test is ignored
        assert (want[compared] == ids["grid"]).all() and counts["grid"] == int(compared.sum()) > 0
        assert (compared & ~rc["hit"][0]).any() and (compared & rc["hit"][0] & (rc["draw"][0] != 2)).any()
    else:
        assert all(n > 0 for n in counts.values()), counts
        winner = np.where(rc["hit"][0], np.array([d.object_id for d in sc.draws], np.uint32)[np.maximum(rc["draw"][0], 0)], 0)
        assert (compared & rc["hit"][0] & (want != winner)).any() and (compared & ~rc["hit"][0] & (want != 0)).any()
