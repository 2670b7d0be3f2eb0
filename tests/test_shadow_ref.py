"""The ShadowMap raster rule on known answers worked by hand, without a GPU: tests/shadow_ref.py is the
restatement ur_shadow_map is held to byte for byte (tests/test_gpu_shadow_map.py runs the same cases on the device), so what it gives
on ties, windings, clipping and snapping is pinned here. All cases draw on an 8 x 8 target under identity matrices: positions are
clip coordinates and, the target being a power of two, land on their target-space coordinates exactly."""
import numpy as np
import pytest

from tests import shadow_ref as R

W = H = 8


def _draw(tris, z=0.5, **kw):
    """One Draw of target-space triangles [((x, y), (x, y), (x, y)), ...]; z a number, or one per vertex."""
    t = np.asarray(tris, np.float64).reshape(-1, 3, 2)
    zs = np.broadcast_to(np.asarray(z, np.float64), t.shape[:2]) if np.ndim(z) < 2 else np.asarray(z, np.float64)
    pos = R.target_to_clip(t[..., 0], t[..., 1], zs, W, H).reshape(-1, 3)
    return R.Draw(R.vertex_buffer(pos), np.arange(pos.shape[0], dtype=np.uint32), **kw)


def _covered(m):
    return {(int(x), int(y)) for y, x in zip(*np.nonzero(m < 1))}


def _count(tris):
    """How many of the triangles cover each centre."""
    n = np.zeros((H, W), np.int64)
    for t in np.asarray(tris, np.float64).reshape(-1, 3, 2):
        f = R.raster_triangle(R.snap(t[:, 0]), R.snap(t[:, 1]), np.float32([0.5] * 3), W, H)
        if f is not None:
            np.add.at(n, (f[0], f[1]), 1)
    return n


CORNER = ((0, 0), (8, 0), (0, 8))               # clockwise on the y-down target: A > 0, drawn
ON_CENTRE = ((2.5, 2.5), (5.5, 2.5), (2.5, 5.5))  # every vertex on a pixel centre
HALF = 0.5 / 256


def hand_cases():
    """name -> (draws, expected stats[0:3]); the GPU test runs them too."""
    nan = _draw([CORNER])
    nan.vertices.view(np.float32)[0] = np.nan
    huge = _draw([CORNER])
    huge.vertices.view(np.float32)[0] = 1e38  # finite, clip w == 1, X overflows
    return {
        "corner": ([_draw([CORNER])], (1, 0, 0)),
        "corner_reversed": ([_draw([CORNER[::-1]])], (0, 0, 0)),
        "quad_main_diagonal": ([_draw([((1, 1), (7, 1), (7, 7)), ((1, 1), (7, 7), (1, 7))], z=[[0.25] * 3, [0.75] * 3])], (2, 0, 0)),
        "quad_other_diagonal": ([_draw([((1, 1), (7, 1), (1, 7)), ((7, 1), (7, 7), (1, 7))], z=[[0.25] * 3, [0.75] * 3])], (2, 0, 0)),
        "vertex_on_centre": ([_draw([ON_CENTRE])], (1, 0, 0)),
        "top_and_bottom_on_centres": ([_draw([((1, 2.5), (6, 2.5), (6, 5.5)), ((1, 2.5), (6, 5.5), (1, 5.5))])], (2, 0, 0)),
        "zero_area": ([_draw([((1, 1), (3, 3), (5, 5))])], (0, 0, 0)),
        "depth_straddles": ([_draw([CORNER], z=[[-0.5, 1.5, 0.5]])], (1, 0, 0)),
        "minus_zero": ([_draw([ON_CENTRE], z=[[-0.0, -0.25, -0.25]])], (1, 0, 0)),
        "w_not_one": ([_draw([CORNER, ON_CENTRE], world=np.diag([1, 1, 1, 2]).astype(np.float32).reshape(-1))], (0, 2, 0)),
        "guard_band_edge": ([_draw([((0, 0), (16384, 0), (0, 8))])], (1, 0, 0)),
        "guard_band_out": ([_draw([((0, 0), (16385, 0), (0, 8)), CORNER])], (1, 0, 1)),
        "nan_position": ([nan], (0, 1, 0)),
        "overflowing_position": ([huge], (0, 0, 1)),
        "snap_ties_to_even": ([_draw([((2.5 + HALF, 1), (6, 1), (2.5 + HALF, 6))])], (1, 0, 0)),
        "snap_ties_to_even_up": ([_draw([((2.5 + 3 * HALF, 1), (6, 1), (2.5 + 3 * HALF, 6))])], (1, 0, 0)),
    }


def _run(name):
    draws, stats = hand_cases()[name]
    m, s = R.shadow_map(draws, R.target_lvp(), W, H)
    assert tuple(int(v) for v in s) == stats, name
    return m


def test_corner_triangle_leaves_its_diagonal_out():
    """(0,0),(8,0),(0,8): the centres with px + py <= 7 lie in the closed triangle, but the eight with px + py == 7 lie ON the edge
    (8,0)->(0,8), whose dy > 0: neither top nor left. The rule gives the 28 centres with px + py <= 6; the top row (a top edge) and the
    left column (a left edge) are far from their edges here and in."""
    m = _run("corner")
    assert _covered(m) == {(x, y) for x in range(8) for y in range(8) if x + y <= 6}
    assert len(_covered(m)) == 28
    assert (m[m < 1] == np.float32(0.5)).all()


def test_reversed_winding_and_zero_area_cover_nothing():
    assert not _covered(_run("corner_reversed"))  # A < 0: counter-clockwise on the target = front-facing, culled (CULL_MODE_FRONT)
    assert not _covered(_run("zero_area"))        # A == 0


@pytest.mark.parametrize("name,tris", [("quad_main_diagonal", [((1, 1), (7, 1), (7, 7)), ((1, 1), (7, 7), (1, 7))]),
                                       ("quad_other_diagonal", [((1, 1), (7, 1), (1, 7)), ((7, 1), (7, 7), (1, 7))])])
def test_quad_split_along_either_diagonal_covers_each_centre_once(name, tris):
    """The diagonal of the square (1,1)-(7,7) passes through six centres: each belongs to exactly one of the two triangles."""
    n = _count(tris)
    want = np.zeros((H, W), np.int64)
    want[1:7, 1:7] = 1
    assert np.array_equal(n, want)
    m = _run(name)
    assert _covered(m) == {(x, y) for x in range(1, 7) for y in range(1, 7)}
    on_diagonal = [(k, k) for k in range(1, 7)] if name == "quad_main_diagonal" else [(k, 7 - k) for k in range(1, 7)]
    # the owner is the triangle that traverses the diagonal upwards (dy < 0, a left edge): the first one's (7,7)->(1,1) (depth 0.25), the
    # second one's (1,7)->(7,1) (depth 0.75)
    owner = {float(m[y, x]) for x, y in on_diagonal}
    assert owner == ({0.25} if name == "quad_main_diagonal" else {0.75}), owner


def test_vertex_exactly_on_a_centre():
    """(2.5,2.5),(5.5,2.5),(2.5,5.5): vertex 0 lies on the top and the left edge (E == 0 on both, both tie-break in): in. Vertex 1 lies
    on the top edge and on the diagonal (not top-left): out, like vertex 2 and the centres (4.5,3.5), (3.5,4.5) between them."""
    m = _run("vertex_on_centre")
    assert _covered(m) == {(2, 2), (3, 2), (4, 2), (2, 3), (3, 3), (2, 4)}


def test_top_edge_on_centres_is_in_bottom_edge_is_out():
    m = _run("top_and_bottom_on_centres")  # the rectangle x in [1, 6], y in [2.5, 5.5]: rows 2, 3, 4 - not 5
    assert _covered(m) == {(x, y) for x in range(1, 6) for y in (2, 3, 4)}


def test_depth_clip_and_minus_zero():
    m = _run("depth_straddles")
    f = R.raster_triangle(R.snap(np.float32([0, 8, 0])), R.snap(np.float32([0, 0, 8])), np.float32([-0.5, 1.5, 0.5]), W, H)
    z = dict(zip(zip(f[1].tolist(), f[0].tolist()), f[2].tolist()))
    assert len(z) == 28 and any(v < 0 for v in z.values()) and any(v > 1 for v in z.values())
    assert _covered(m) == {k for k, v in z.items() if 0 <= v < 1} and 0 < len(_covered(m)) < 28
    assert ((m >= 0) & (m <= 1)).all()
    # z0 = -0 at a vertex on a centre, slopes negative: the fragment's depth is -0 (0 * k = -0, -0 + -0 = -0): it passes the clip and is stored as +0
    m = _run("minus_zero")
    f = R.raster_triangle(R.snap(np.float32([2.5, 5.5, 2.5])), R.snap(np.float32([2.5, 2.5, 5.5])), np.float32([-0.0, -0.25, -0.25]), W, H)
    at = [i for i in range(f[0].size) if (f[1][i], f[0][i]) == (2, 2)]
    assert len(at) == 1 and f[2][at[0]] == 0 and np.signbit(f[2][at[0]])
    assert _covered(m) == {(2, 2)} and m.view(np.uint32)[2, 2] == 0


def test_unsupported_and_dropped_triangles():
    for name in ("w_not_one", "nan_position", "overflowing_position"):
        assert not _covered(_run(name)), name  # (a NaN position makes clip w NaN, which is not 1.0f: unsupported, not dropped)
    assert len(_covered(_run("guard_band_edge"))) == 64  # a vertex AT 16384 px is drawn: its diagonal passes outside the target
    assert _covered(_run("guard_band_out")) == {(x, y) for x in range(8) for y in range(8) if x + y <= 6}  # only its second triangle
    # a command as a whole: another index format, a stride below 12
    d = _draw([CORNER, ON_CENTRE])
    d.index_format = 57
    assert tuple(R.shadow_map([d], R.target_lvp(), W, H)[1]) == (0, 2, 0)
    d = _draw([CORNER])
    d.stride = 8
    assert tuple(R.shadow_map([d], R.target_lvp(), W, H)[1]) == (0, 1, 0)
    d = _draw([CORNER, CORNER])
    d.indices = d.indices[:5]  # the second triangle's last index lies outside the view
    d.index_count = 6
    assert tuple(R.shadow_map([d], R.target_lvp(), W, H)[1]) == (1, 1, 0)
    d = _draw([CORNER])
    d.instance_count = 0
    m, s = R.shadow_map([d], R.target_lvp(), W, H)
    assert not _covered(m) and tuple(s) == (0, 0, 0)


def test_snapping_rounds_ties_to_even():
    assert R.snap(np.float32([2.5 + HALF, 2.5 + 3 * HALF, -HALF, HALF, 3 * HALF])).tolist() == [640, 642, 0, 0, 2]
    # 640 is the centre of column 2: the left edge ties in. Rounding the tie up (641) would leave the column out.
    assert _covered(_run("snap_ties_to_even")) >= {(2, 1), (2, 2)}
    assert not any(x == 2 for x, _ in _covered(_run("snap_ties_to_even_up")))


def test_selection_restated():
    assert R.selected_slots(5) == [0, 1, 2, 3, 4]
    assert R.selected_slots(5, visible=(np.array([12, 10, 99, 14], np.uint32), 3), index_base=10) == [2, 0]
    assert R.selected_slots(5, visible=(np.array([1], np.uint32), 0)) == []
    assert R.selected_slots(6, ranges=(np.array([0, 2, 2, 6]), np.array([1, 0, 9]))) == [0, 2, 3, 4, 5]


def test_fp32_depth_is_close_to_float64_on_the_soups():
    """max |z_fp32 - z_float64| over the covered fragments of the GPU test's soups against the bound the restatement records: 4 x the
    measured maximum, rounded up to a power of two times 2^-24 (the seeds are a sample)."""
    worst = 0.0
    for w, h, seed in ((64, 64, 1), (257, 130, 2), (2048, 2048, 3)):
        e = R.depth_error(R.soup(w, h, seed), R.target_lvp(), w, h)
        print(f"soup {w}x{h} seed {seed}: max |z_fp32 - z_fp64| = {e:.3e} = {e * 2 ** 24:.2f} x 2^-24")
        worst = max(worst, e)
    bound = R.DEPTH_ERROR_BOUND
    assert bound == 2.0 ** np.ceil(np.log2(4 * R.MEASURED_DEPTH_ERROR * 2 ** 24)) * 2.0 ** -24
    assert worst <= bound, (worst, bound)
    assert abs(worst - R.MEASURED_DEPTH_ERROR) <= 0.01 * R.MEASURED_DEPTH_ERROR  # the recorded figure is this measurement
