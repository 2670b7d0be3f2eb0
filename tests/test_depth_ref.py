"""The DepthPrepass rule as tests/depth_ref.py restates it, pinned by answers worked out by hand on an 8 x 8
target under hand_camera (clip = (x, y, 1/8, z): every operation of the cases below is exact), the soup conditions of the GPU test, and
the accuracy of the fp32 depth against float64."""
import numpy as np
import pytest

from tests import depth_ref as R
from tests import shadow_ref as S

W = H = 8
N = R.NEAR


def _draw(tris, **kw):
    """tris: [((X, Y, z), (X, Y, z), (X, Y, z))] - target position and view depth of each vertex"""
    pos = np.array([R.at(x, y, z, W, H) for t in tris for (x, y, z) in t], np.float32)
    return R.Draw(R.vertex_buffer(pos), np.arange(pos.shape[0], dtype=np.uint32), **kw)


def _clip(tris):
    """Triangles given by clip coordinates (cx, cy, cw) per vertex: position (cx, cy, cw) under hand_camera."""
    pos = np.array([v for t in tris for v in t], np.float32)
    return R.Draw(R.vertex_buffer(pos), np.arange(pos.shape[0], dtype=np.uint32))


# section 3.7's tie triangle, its vertices 1 and 2 exchanged: counter-clockwise on the target (y down), A < 0, a front face
CORNER = ((0, 0, 0.25), (0, 8, 0.25), (8, 0, 0.25))
# a = target (0,0), b = target (0,8), both at w = 1/4 (d = 1/8); c = clip (1/4, 1/4) at w = 0 (d = -1/8): t = 1/2 on both edges.
# p = (b + c) / 2 = clip (0, 0, w 1/8) = target (4, 4); q = (a + c) / 2 = clip (0, 1/4, w 1/8) = NDC (0, 2) = target (4, -4).
ONE_OUT = ((-0.25, 0.25, 0.25), (-0.25, -0.25, 0.25), (0.25, 0.25, 0.0))
# a = target (0,0) at w = 1/4; b = clip (0, -1/2), c = clip (1/2, 0), both at w = 0: p = (a + b) / 2 = clip (-1/8, -1/8, w 1/8) = target
# (0, 8), q = (a + c) / 2 = clip (1/8, 1/8, w 1/8) = target (8, 0)
TWO_OUT = ((-0.25, 0.25, 0.25), (0.0, -0.5, 0.0), (0.5, 0.0, 0.0))
# two of its three vertices on the near plane (depth 1.0), found by search: three of its ten fragments round to 1.0000001
ROUNDS_ABOVE_ONE = ((5, 0, 6.0), (0.5, 1.5, N), (3, 4, N))


def _shared_edge():
    """Two triangles sharing the edge a-c, a in front of the near plane and c behind the eye, none of the numbers round: a, b, e lie
    around the target at w = 0.3 and the cut points beyond its bottom right, so the two clipped triangles cover the target between them."""
    a, b, e, c = (-1.8, 1.8, 0.3), (-1.8, -2.7, 0.3), (2.7, 1.8, 0.3), (4.171, -4.171, -0.1)
    return [(a, b, c), (a, c, e)]


def hand_cases():
    """name -> (draws, expected stats[0:6]); the GPU test runs them too."""
    nan = _draw([CORNER])
    nan.vertices.view(np.float32)[0] = np.nan
    g = float(R.GUARD_BAND)
    return {
        "corner": ([_draw([CORNER])], (1, 0, 0, 0, 0, 0)),
        "corner_reversed": ([_draw([CORNER[::-1]])], (0, 0, 0, 0, 0, 0)),
        "zero_area": ([_draw([((1, 1, 0.25), (3, 3, 0.5), (5, 5, 1.0))])], (0, 0, 0, 0, 0, 0)),
        "one_vertex_behind": ([_clip([ONE_OUT])], (2, 0, 0, 0, 1, 0)),
        "two_vertices_behind": ([_clip([TWO_OUT])], (1, 0, 0, 0, 1, 0)),
        "shared_cut_edge": ([_clip(_shared_edge())], (4, 0, 0, 0, 2, 0)),
        "wholly_behind": ([_clip([((-0.25, 0.25, 0.0625), (-0.25, -0.25, 0.0), (0.25, 0.25, -1.0))])], (0, 0, 0, 0, 0, 1)),
        "on_the_near_plane": ([_draw([tuple((x, y, N) for x, y, _ in CORNER)])], (1, 0, 0, 0, 0, 0)),
        "clip_z_zero": ([_draw([CORNER], world=np.diag([1, 1, 1, 0]).astype(np.float32).reshape(-1))], (0, 1, 0, 0, 0, 0)),
        "clip_z_negative": ([_draw([CORNER, CORNER], world=np.diag([1, 1, 1, -1]).astype(np.float32).reshape(-1))], (0, 2, 0, 0, 0, 0)),
        "nan_position": ([nan], (0, 1, 0, 0, 0, 0)),
        "guard_band_edge": ([_draw([((0, 0, 0.25), (0, 8, 0.25), (g, 0, 0.25))])], (1, 0, 0, 0, 0, 0)),
        "guard_band_out": ([_draw([((0, 0, 0.25), (0, 8, 0.25), (g + 8, 0, 0.25)), CORNER])], (1, 0, 1, 0, 0, 0)),
        "rounds_above_one": ([_draw([ROUNDS_ABOVE_ONE])], (1, 0, 0, 0, 0, 0)),
        "nearer_wins": ([_draw([CORNER, tuple((x, y, 0.5) for x, y, _ in CORNER), tuple((x, y, 0.125 * 1.5) for x, y, _ in CORNER)])], (3, 0, 0, 0, 0, 0)),
    }


def _run(name, flags=0):
    draws, stats = hand_cases()[name]
    m, s = R.depth_prepass(draws, *R.hand_camera(W, H), W, H, flags=flags)
    assert tuple(int(v) for v in s) == stats, name
    return m


def _covered(m):
    return {(int(x), int(y)) for y, x in np.argwhere(m > 0)}


def test_corner_triangle_mirrored_for_the_new_facing():
    """(0,0),(0,8),(8,0) is counter-clockwise on the target: A < 0, drawn. Taken as (u0, u2, u1) it is section 3.7's tie triangle: the 28
    centres with px + py <= 6, the eight on the diagonal (neither top nor left) out. Depth 1/8 / 1/4 = 0.5 everywhere."""
    m = _run("corner")
    assert _covered(m) == {(x, y) for x in range(8) for y in range(8) if x + y <= 6}
    assert (m[m > 0] == np.float32(0.5)).all()
    assert not _covered(_run("corner_reversed"))  # clockwise on the target: a back face (CULL_MODE_BACK)
    assert not _covered(_run("zero_area"))


def test_one_vertex_behind_the_near_plane():
    """The polygon is a (0,0), b (0,8), p (4,4), q (4,-4), cut along a-p: (a, b, p) covers px < py, px + py <= 6 (its edge p->b is
    neither top nor left), (a, p, q) covers py <= px <= 3 - the centres on the diagonal a-p are its own, the edge p->a of its reordered
    form runs upwards: a left edge. a and b have depth 1/2, p and q exactly 1: the plane is 1/2 + X / 8 in both triangles, exactly."""
    poly, emit, n_out = R.near_clip(R.project(np.array(ONE_OUT, np.float32), R.IDENTITY, *R.hand_camera(W, H)).reshape(1, 3, 4))
    assert int(emit[0]) == 2 and int(n_out[0]) == 1
    X, Y, Z = R.viewport(poly, W, H)
    assert list(zip(X[0].tolist(), Y[0].tolist(), Z[0].tolist())) == [(0, 0, 0.5), (0, 8, 0.5), (4, 4, 1.0), (4, -4, 1.0)]
    m = _run("one_vertex_behind")
    first = {(x, y) for x in range(8) for y in range(8) if x < y and x + y <= 6}
    second = {(x, y) for x in range(4) for y in range(x + 1)}
    assert len(first) == 12 and len(second) == 10 and _covered(m) == first | second
    for x, y in first | second:
        assert m[y, x] == np.float32(0.5 + (x + 0.5) / 8)


def test_two_vertices_behind_the_near_plane():
    """The triangle left is a (0,0), p (0,8), q (8,0) with depths 1/2, 1, 1: the 28 centres of the corner case, depth 1/2 + (X + Y) / 16."""
    poly, emit, n_out = R.near_clip(R.project(np.array(TWO_OUT, np.float32), R.IDENTITY, *R.hand_camera(W, H)).reshape(1, 3, 4))
    assert int(emit[0]) == 1 and int(n_out[0]) == 2
    X, Y, Z = R.viewport(poly, W, H)
    assert list(zip(X[0, :3].tolist(), Y[0, :3].tolist(), Z[0, :3].tolist())) == [(0, 0, 0.5), (0, 8, 1.0), (8, 0, 1.0)]
    m = _run("two_vertices_behind")
    assert _covered(m) == {(x, y) for x in range(8) for y in range(8) if x + y <= 6}
    for x, y in _covered(m):
        assert m[y, x] == np.float32(0.5 + (x + y + 1) / 16)


def test_two_triangles_sharing_a_cut_edge():
    """The new vertex on a-c has the same bits in both triangles (it is computed from a towards c in both), so the four emitted triangles
    tile the polygon: every centre of the target is covered exactly once - none uncovered, none drawn twice with two depths."""
    tris = _shared_edge()
    cam = R.hand_camera(W, H)
    polys = [R.near_clip(R.project(np.array(t, np.float32), R.IDENTITY, *cam).reshape(1, 3, 4))[0][0] for t in tris]
    # (a, b, c): a, b, p(b->c), q(a->c); (a, c, e) rotated to (e, a, c): e, a, p(a->c), q(e->c)
    assert np.array_equal(polys[0][3].view(np.uint32), polys[1][2].view(np.uint32))
    assert np.array_equal(polys[0][0].view(np.uint32), polys[1][1].view(np.uint32))
    count = np.zeros((H, W), np.int64)
    for poly in polys:
        X, Y, Z = R.viewport(poly[None], W, H)
        for e in range(2):
            u = [0, 2 + e, 1 + e]
            py, px, _ = S.raster_triangle(S.snap(X[0, u]), S.snap(Y[0, u]), Z[0, u], W, H)
            np.add.at(count, (py, px), 1)
    assert (count == 1).all(), count
    m = _run("shared_cut_edge")
    assert (m > 0).all() and (m < 1).all()


def test_behind_unsupported_and_guard_band():
    assert not _covered(_run("wholly_behind"))
    m = _run("on_the_near_plane")  # d == 0 is inside: the corner case at depth exactly 1.0
    assert _covered(m) == {(x, y) for x in range(8) for y in range(8) if x + y <= 6} and (m[m > 0] == 1.0).all()
    for name in ("clip_z_zero", "clip_z_negative", "nan_position"):
        assert not _covered(_run(name)), name
    edge = _run("guard_band_edge")  # a vertex exactly on the band, 2^21 px: drawn, and the edge functions are still exact
    f = S.raster_triangle(S.snap(np.float32([0, float(R.GUARD_BAND), 0])), S.snap(np.float32([0, 0, 8])), np.float32([0.5] * 3), W, H)
    assert _covered(edge) == set(zip(f[1].tolist(), f[0].tolist())) and len(_covered(edge)) == 64
    out = _run("guard_band_out")  # one px beyond: dropped whole; the corner triangle beside it is drawn
    assert _covered(out) == {(x, y) for x in range(8) for y in range(8) if x + y <= 6}


def test_depth_is_clamped_at_one_and_the_maximum_wins():
    pos = np.array([R.at(x, y, z, W, H) for x, y, z in ROUNDS_ABOVE_ONE], np.float32)
    poly, _, _ = R.near_clip(R.project(pos, R.IDENTITY, *R.hand_camera(W, H)).reshape(1, 3, 4))
    X, Y, Z = R.viewport(poly, W, H)
    u = [0, 2, 1]
    raw = S.raster_triangle(S.snap(X[0, u]), S.snap(Y[0, u]), Z[0, u], W, H)[2]
    assert (Z[0, :3] <= 1).all() and raw.size == 10 and int((raw > 1).sum()) == 3 and raw.max() == np.float32(1.0000001)
    m = _run("rounds_above_one")
    assert len(_covered(m)) == 10 and m.max() == np.float32(1.0) and int((m == 1).sum()) == 3
    m = _run("nearer_wins")  # view depths 1/4, 1/2, 3/16 over the same centres: 1/8 / (3/16) = 2/3 is the nearest
    assert (m[m > 0] == np.float32(0.125) / np.float32(0.1875)).all() and len(_covered(m)) == 28


@pytest.mark.parametrize("name", sorted(hand_cases()))
def test_d24_bytes_are_the_quantised_float_result(name):
    from unclerenderer_amd import synth
    plain, q = _run(name), _run(name, R.QUANTIZE_D24)
    assert np.array_equal(q.view(np.uint32), synth.quantize_d24(plain).view(np.uint32))


# ---- the soups of the GPU test ---------------------------------------------------------------------------------------------------

_SOUP = {}


def soup_reference(w, h, seed, dirty=False):
    """(draws, view, projection, target, stats, info, errors) of a soup, computed once and left unchanged."""
    key = (w, h, seed, dirty)
    if key not in _SOUP:
        draws = R.soup(w, h, seed, dirty=dirty)
        view, proj = R.soup_camera(w, h)
        info, errs = {}, []
        m, s = R.depth_prepass(draws, view, proj, w, h, info=info, error_out=errs)
        m.setflags(write=False)
        _SOUP[key] = (draws, view, proj, m, s, info, max(errs))
    return _SOUP[key]


@pytest.mark.parametrize("w,h,seed", R.SOUPS)
def test_clean_soup_conditions(w, h, seed):
    """What the GPU test's byte equality is worth: the picture is not empty and every path of the kernel is taken."""
    _, _, _, m, s, info, _ = soup_reference(w, h, seed)
    assert s[1] == 0 and s[2] == 0
    assert (m > 0).mean() >= 0.25
    assert info["one_out"] >= 50 and info["two_out"] >= 50 and s[4] == info["one_out"] + info["two_out"]
    assert s[5] >= 20
    assert info["own"] >= 1 and info["wave"] >= 1
    # a large triangle has a bounding box of more than 64 8 x 8 stamps, clamped to the target: a 64 x 64 target has 64 stamps in all
    stamps = ((w + 7) // 8) * ((h + 7) // 8)
    assert info["large"] >= 1 if stamps > 64 else info["large"] == 0


@pytest.mark.parametrize("w,h,seed", R.SOUPS)
def test_dirty_soup_conditions(w, h, seed):
    _, _, _, _, s, _, _ = soup_reference(w, h, R.DIRTY_SEED, dirty=True)
    assert s[1] >= 20 and s[2] >= 20 and s[0] > 0


def test_depth_accuracy_over_the_soups():
    """max |z_fp32 - z_float64| over every covered fragment of the three soups, the float64 depth from the same snapped integers and
    per-vertex depths: the documented maximum (depth_ref's docstring), and the bound of 4 x that, rounded up to a power of
    two."""
    worst = max(soup_reference(w, h, seed)[6] for w, h, seed in R.SOUPS)
    print(f"max |z_fp32 - z_float64| = {worst:.3e} = {worst * 2 ** 24:.2f} x 2^-24")
    assert worst <= R.DEPTH_ERROR_BOUND
    assert abs(worst - R.MEASURED_DEPTH_ERROR) <= 0.01 * R.MEASURED_DEPTH_ERROR, "the documented maximum is not the measured one"
    assert R.DEPTH_ERROR_BOUND == 2.0 ** np.ceil(np.log2(4 * R.MEASURED_DEPTH_ERROR))
    # and the picture itself: the fp32 target against the float64 target
    w, h, seed = R.SOUPS[0]
    draws, view, proj, m, _, _, _ = soup_reference(w, h, seed)
    m64, _ = R.depth_prepass(draws, view, proj, w, h, depth="fp64")
    assert np.abs(m.astype(np.float64) - m64).max() <= R.DEPTH_ERROR_BOUND
