"""The float64 ray caster (tests/raycast_ref.py) against hand-worked answers, its left-out share under the cap on every scene, and every
raster restatement (shadow_map, depth_prepass, gbuffer_pass) held to it on connected meshes under real cameras. The GPU files assert that
the kernels equal the restatements byte for byte, so this file holds the kernels transitively; tests/test_gpu_raster_raycast.py holds
them directly. Four planted errors show that the comparison bites."""
import numpy as np
import pytest

from tests import depth_ref as D
from tests import gbuffer_ref as G
from tests import raycast_ref as R
from tests import shadow_ref as S

pytestmark = pytest.mark.usefixtures("urlib")  # the scenes' cameras come from the library's host math

SCENES = sorted(R.CAMERA_SCENES)
IDENTITY = np.eye(4, dtype=np.float32).reshape(-1)
NEAR = 0.125
HAND_PROJ = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, NEAR, 0], np.float32)  # 90 degrees, square: clip = (x, y, NEAR, z)


def _one_triangle(p):
    return [G.GDraw(G.vertex_buffer(p), np.arange(3, dtype=np.uint32), object_id=1)]


def report(record_property, what, res):
    for k, (fails, worst) in sorted(res.items()):
        record_property(f"{what}: {k}: largest error / tolerance", round(float(worst), 4))
    print(what, {k: (f, round(float(x), 4)) for k, (f, x) in sorted(res.items())})


# ---- hand-worked answers ----------------------------------------------------------------------------------------------------------------

FACING = [(-20, -10, 2), (20, -10, 2), (0, 30, 2)]  # (v1 - v0) x (v2 - v0) = (0, 0, 1600): away from a viewer at the origin - the front


def test_facing_triangle_has_known_depths():
    """The plane z = 2 fills the view: depth NEAR / 2, view depth -2 and the default normal (0, 0, -1) at every one of the 9 x 64 rays."""
    rc = R.cast(_one_triangle(FACING), 8, 8, IDENTITY, HAND_PROJ)
    assert rc["hit"].all() and (rc["draw"] == 0).all() and (rc["tri"] == 0).all()
    assert np.allclose(rc["depth"], NEAR / 2, rtol=0, atol=1e-15) and np.allclose(rc["view_depth"], -2.0, rtol=0, atol=1e-14)
    assert np.allclose(rc["normal"], [0, 0, -1], rtol=0, atol=1e-15) and np.allclose(rc["albedo"], 1.0, rtol=0, atol=1e-15)
    compared, any_hit, share = R.classify(rc)
    assert compared.all() and any_hit.all() and share == 0.0


def test_other_winding_gives_nothing():
    rc = R.cast(_one_triangle([FACING[0], FACING[2], FACING[1]]), 8, 8, IDENTITY, HAND_PROJ)
    assert not rc["hit"].any() and R.classify(rc)[0].all()
    # ... and under a light the same pair swaps: CULL_MODE_FRONT keeps what the camera drops
    lvp = np.array([0.25, 0, 0, 0, 0, 0.25, 0, 0, 0, 0, 0.25, 0, 0, 0, 0, 1], np.float32)  # x, y in [-4, 4], depth = z / 4
    assert not R.cast(_one_triangle(FACING), 8, 8, lvp=lvp)["hit"].any()
    back = R.cast(_one_triangle([FACING[0], FACING[2], FACING[1]]), 8, 8, lvp=lvp)
    assert back["hit"].all() and np.allclose(back["depth"], 0.5, rtol=0, atol=1e-15)


def test_near_plane_straddler_hits_only_in_front():
    """A floor y = -1/16 from z = -1 to z = 3, seen from above. The ray of row py has NDC y = 1 - (py + 0.5) / 8 and meets the floor at
    view depth z = -(1/16) / y: rows 0-7 look up, rows 8-11 meet it at z = 1, 1/3, 1/5, 1/7, rows 12-15 at 1/9 ... 1/15, inside NEAR =
    1/8 - those are gone."""
    rc = R.cast(_one_triangle([(-10, -0.0625, -1), (10, -0.0625, -1), (0, -0.0625, 3)]), 16, 16, IDENTITY, HAND_PROJ)
    rows = rc["hit"][0].all(axis=1)
    assert rows.tolist() == [8 <= py <= 11 for py in range(16)] and not rc["hit"][0][~rows].any()
    z = 1.0 / np.array([1.0, 3.0, 5.0, 7.0])
    assert np.allclose(rc["view_depth"][0][8:12], -z[:, None], rtol=1e-13, atol=0)
    assert np.allclose(rc["depth"][0][8:12], (NEAR / z)[:, None], rtol=1e-13, atol=0)
    assert (rc["view_depth"][rc["hit"]] <= -NEAR).all()


# ---- the scenes ---------------------------------------------------------------------------------------------------------------------------

def test_scenes_are_what_they_claim():
    pos, faces = R.icosphere_mesh()
    assert pos.shape == (162, 3) and faces.shape == (320, 3)
    tpos, _, tfaces = R.torus_mesh()
    assert tpos.shape == (16 * 12, 3) and tfaces.shape == (2 * 16 * 12, 3)
    for f in (faces, tfaces):  # closed: every edge is shared by exactly two triangles, once in each direction
        e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
        assert len({tuple(x) for x in e.tolist()}) == e.shape[0] and {tuple(x) for x in e.tolist()} == {tuple(x) for x in e[:, ::-1].tolist()}
    for w, h in R.TARGETS:
        sc = R.strip_scene(w, h)
        assert sc.draws[0].count() == 3 * 32 and sc.draws[1].count() == 3 * 2
        info = {}
        _, stats = D.depth_prepass(sc.draws, sc.view, sc.proj, w, h, info=info)
        assert info["one_out"] >= 2 and info["two_out"] >= 2 and stats[5] >= 1, (stats.tolist(), info)  # both cuts, and wholly behind
        # the queue's triangles: more than 64 stamps of 8 x 8, which only a target above 64 x 64 has room for
        assert info["large"] >= (2 if (w, h) != (64, 64) else 0), info
        lit = R.shadow_scene(w, h)
        assert S.shadow_map(lit.draws, lit.lvp, w, h)[1].tolist()[1:] == [0, 0]  # clip w is 1 everywhere, nothing dropped


@pytest.mark.parametrize("w,h", R.TARGETS)
@pytest.mark.parametrize("name", SCENES + ["shadow"])
def test_left_out_share_is_under_the_cap(record_property, name, w, h):
    _, rc = R.cast_scene(name, w, h)
    compared, any_hit, share = R.classify(rc)
    record_property(f"{name} {w}x{h}: left-out share", round(share, 4))
    print(f"{name} {w}x{h}: {int(any_hit.sum())} texels hit, {int((any_hit & compared).sum())} compared, left out {share:.4f}")
    assert any_hit.sum() >= w * h // 8  # the scene fills a good part of the target
    assert share <= R.LEFT_OUT_CAP


# ---- the restatements against the ray caster -----------------------------------------------------------------------------------------------

_RESTATED = {}


def restated(name, w, h, order=1):
    """(depth, gbuffer dict) of the restatements over a camera scene, cached; order = -1 draws the scene's draws backwards."""
    if (name, w, h, order) not in _RESTATED:
        sc, _ = R.cast_scene(name, w, h)
        draws = sc.draws[::order]
        depth, _ = D.depth_prepass(draws, sc.view, sc.proj, w, h)
        out = G.gbuffer_pass(draws, sc.view, sc.proj, depth, w, h)
        _RESTATED[(name, w, h, order)] = (depth, out)
    return _RESTATED[(name, w, h, order)]


@pytest.mark.parametrize("w,h", R.TARGETS)
def test_shadow_map_agrees(record_property, w, h):
    sc, rc = R.cast_scene("shadow", w, h)
    res = R.compare_depth(rc, S.shadow_map(sc.draws, sc.lvp, w, h)[0], S.DEPTH_ERROR_BOUND, 1.0)
    report(record_property, f"shadow_map, shadow {w}x{h}", res)
    assert R.failures(res) == 0, res


@pytest.mark.parametrize("w,h", R.TARGETS)
@pytest.mark.parametrize("name", SCENES)
def test_depth_prepass_agrees(record_property, name, w, h):
    _, rc = R.cast_scene(name, w, h)
    res = R.compare_depth(rc, restated(name, w, h)[0], D.DEPTH_ERROR_BOUND, 0.0)
    report(record_property, f"depth_prepass, {name} {w}x{h}", res)
    assert R.failures(res) == 0, res


@pytest.mark.parametrize("w,h", R.TARGETS)
@pytest.mark.parametrize("name", SCENES)
def test_gbuffer_pass_agrees(record_property, name, w, h):
    sc, rc = R.cast_scene(name, w, h)
    res = R.compare_gbuffer(rc, restated(name, w, h)[1], sc.draws, G.A_ULPS_BOUND, G.C_CODES_BOUND)
    report(record_property, f"gbuffer_pass, {name} {w}x{h}", res)
    assert R.failures(res) == 0, res


@pytest.mark.parametrize("w,h", R.TARGETS)
def test_two_draws_in_the_other_order(record_property, w, h):
    """Drawn torus first: the ray caster knows no order, and on the compared texels neither does the result."""
    sc, rc = R.cast_scene("two draws", w, h)
    depth, out = restated("two draws", w, h, -1)
    res = R.compare_gbuffer(rc, out, sc.draws, G.A_ULPS_BOUND, G.C_CODES_BOUND)
    res["depth"] = R.compare_depth(rc, depth, D.DEPTH_ERROR_BOUND, 0.0)["depth"]
    report(record_property, f"gbuffer_pass, two draws backwards {w}x{h}", res)
    assert R.failures(res) == 0, res
    compared = R.classify(rc)[0]
    forward = restated("two draws", w, h)[1]
    for k in ("A", "B", "C", "hdr", "object_id"):
        assert np.array_equal(out[k][compared], forward[k][compared]), k
    assert set(out["object_id"][compared].tolist()) == {0, 7, 0x80000021}  # both draws are seen


# ---- detectors: a planted error must fail the comparison ----------------------------------------------------------------------------------

W0, H0 = R.TARGETS[0]


def _unshared(d, swap_colours=False, without=None):
    """The draw with three vertices of its own per triangle: optionally the colours of corners 1 and 2 exchanged, or one triangle gone."""
    v = np.ascontiguousarray(d.vertices).view(np.float32).reshape(-1, 16)
    f = np.asarray(d.indices, np.int64).reshape(-1, 3)
    if without is not None:
        f = np.delete(f, without, axis=0)
    nv = v[f.reshape(-1)].copy()
    if swap_colours:
        nv[:, 12:15] = v[f[:, [0, 2, 1]].reshape(-1), 12:15]
    return G.GDraw(nv.reshape(-1).view(np.uint8).copy(), np.arange(nv.shape[0], dtype=np.uint32), d.world, base_color=d.base_color,
                   emissive=d.emissive, metallic=d.metallic, roughness=d.roughness, object_id=d.object_id)


def _restate(sc, draws):
    depth, _ = D.depth_prepass(draws, sc.view, sc.proj, W0, H0)
    return depth, G.gbuffer_pass(draws, sc.view, sc.proj, depth, W0, H0)


def test_detector_unshared_mesh_alone_changes_nothing():
    sc, rc = R.cast_scene("icosphere", W0, H0)
    depth, out = _restate(sc, [_unshared(sc.draws[0])])
    assert R.failures(R.compare_gbuffer(rc, out, sc.draws, G.A_ULPS_BOUND, G.C_CODES_BOUND)) == 0
    assert R.failures(R.compare_depth(rc, depth, D.DEPTH_ERROR_BOUND, 0.0)) == 0


def test_detector_swapped_albedo_vertices():
    sc, rc = R.cast_scene("icosphere", W0, H0)
    _, out = _restate(sc, [_unshared(sc.draws[0], swap_colours=True)])
    res = R.compare_gbuffer(rc, out, sc.draws, G.A_ULPS_BOUND, G.C_CODES_BOUND)
    assert res["C"][0] > 0 and res["C"][1] > 1.0, res
    assert all(res[k][0] == 0 for k in ("A", "B", "hdr", "object_id", "covered")), res  # and nothing else is blamed


def test_detector_weight_rows_towards_the_wrong_vertex(monkeypatch):
    """The near clip's new vertices weighted t at the inside vertex and 1 - t at the outside one, on the strip."""
    right = G.near_clip

    def wrong(c):
        poly, emit, n_out, B = right(c)
        new = ((B > 0) & (B < 1)).any(axis=2)
        B = B.copy()
        B[new] = np.where(B[new] > 0, 1 - B[new], 0)
        return poly, emit, n_out, B

    sc, rc = R.cast_scene("near-plane strip", W0, H0)
    monkeypatch.setattr(G, "near_clip", wrong)
    _, out = _restate(sc, sc.draws)
    res = R.compare_gbuffer(rc, out, sc.draws, G.A_ULPS_BOUND, G.C_CODES_BOUND)
    assert res["A"][0] > 0 and res["C"][0] > 0, res


def test_detector_crack():
    sc, rc = R.cast_scene("icosphere", W0, H0)
    compared = R.classify(rc)[0] & rc["hit"][0]
    ys, xs = np.nonzero(compared)
    k = np.argmin((ys - ys.mean()) ** 2 + (xs - xs.mean()) ** 2)  # a compared texel in the middle of the sphere
    gone = int(rc["tri"][0][ys[k], xs[k]])
    depth, out = _restate(sc, [_unshared(sc.draws[0], without=gone)])
    res = R.compare_gbuffer(rc, out, sc.draws, G.A_ULPS_BOUND, G.C_CODES_BOUND)
    assert res["covered"][0] > 0 and res["object_id"][0] > 0, res
    assert R.compare_depth(rc, depth, D.DEPTH_ERROR_BOUND, 0.0)["covered"][0] > 0


def test_detector_offset_depth_plane():
    sc, rc = R.cast_scene("icosphere", W0, H0)
    depth = restated("icosphere", W0, H0)[0]
    off = np.where(depth > 0, depth + np.float32(8.0 * D.DEPTH_ERROR_BOUND), depth).astype(np.float32)
    res = R.compare_depth(rc, off, D.DEPTH_ERROR_BOUND, 0.0)
    assert res["depth"][0] > 0 and res["depth"][1] > 1.0, res
    w, h = R.TARGETS[1]  # (the light's depth is steep on 64 x 64: its 9-ray spread alone exceeds 8 bounds there)
    lit, lrc = R.cast_scene("shadow", w, h)
    m = S.shadow_map(lit.draws, lit.lvp, w, h)[0]
    res = R.compare_depth(lrc, np.where(m < 1, m - np.float32(8.0 * S.DEPTH_ERROR_BOUND), m), S.DEPTH_ERROR_BOUND, 1.0)
    assert res["depth"][0] > 0, res
