"""ur_gbuffer_pass_masked on the GPU: keys, keys64, depth, won, A, B, C, HDR and both stats6 (except [3], structural) are byte-equal to
tests/gbuffer_mask_ref.py, the rule of DESIGN.md section 3.11; NaN is compared by NaN-ness."""
import numpy as np
import pytest

from tests import depth_ref as D
from tests import gbuffer_mask_ref as M
from tests import gbuffer_ref as G
from tests import gbuffer_tex_ref as X
from tests.gbuffer_gpu import device_draws
from tests.gbuffer_mask_gpu import Selections, run, same_masked
from tests.gbuffer_tex_gpu import device_materials
from tests.test_gbuffer_mask_ref import H as HAND_H
from tests.test_gbuffer_mask_ref import W as HAND_W
from tests.test_gbuffer_mask_ref import hand_cases, run_case, soup_reference

pytestmark = pytest.mark.gpu

_DEVICE = {}


def _soup(w, h, seed):
    """The soup's reference and its device copy (draws, materials, range selections), uploaded once."""
    key = (w, h, seed)
    if key not in _DEVICE:
        draws, mats, opaque, masked, *_ = soup_reference(w, h, seed)
        dd = device_draws(draws)
        _DEVICE[key] = (dd, device_materials(mats), Selections(dd, [s for _, s in opaque], [s for _, s in masked]))
    return soup_reference(w, h, seed), _DEVICE[key]


@pytest.mark.parametrize("flags", [0, G.QUANTIZE_D24])
@pytest.mark.parametrize("name", sorted(hand_cases()))
def test_hand_cases(hotpath, name, flags):
    case = hand_cases()[name]
    draws, mats, opaque, masked = case
    want, depth = run_case(case, flags=flags)
    dd = device_draws(draws)
    got = run(hotpath, Selections(dd, opaque, masked), device_materials(mats), *D.hand_camera(HAND_W, HAND_H), depth, HAND_W, HAND_H, flags=flags)
    same_masked(got, want, depth, name)


@pytest.mark.parametrize("w,h,seed", M.SOUPS)
def test_soups(hotpath, w, h, seed):
    """With room in the large-triangle queue, with a queue of one entry and without one."""
    (_, _, _, _, view, proj, depth, want), (_, mats, sel) = _soup(w, h, seed)
    try:
        for reserve in (1 << 16, 1, 0):
            hotpath.raster_reserve(reserve)
            got = run(hotpath, sel, mats, view, proj, depth, w, h)
            same_masked(got, want, depth, f"soup {w}x{h}, reserve {reserve}")
    finally:
        hotpath.raster_reserve(0)


@pytest.mark.parametrize("bands", [((0, 65), (65, 65)), ((0, 37), (37, 41), (78, 52))])
def test_bands_against_the_whole_frame(hotpath, bands):
    """257 x 130 in bands: every band's targets, keys64 and depth rows are the whole frame's, and depth outside the band is untouched."""
    w, h, seed = M.SOUPS[1]
    (_, _, _, _, view, proj, depth, want), (_, mats, sel) = _soup(w, h, seed)
    hotpath.raster_reserve(4096)
    try:
        for row0, rows in bands:
            got = run(hotpath, sel, mats, view, proj, depth, w, h, row0, rows)
            same_masked(got, want, depth, f"rows [{row0}, {row0 + rows})", row0, rows)
    finally:
        hotpath.raster_reserve(0)


@pytest.mark.parametrize("w,h,seed", M.SOUPS)
def test_soups_d24(hotpath, w, h, seed):
    (draws, ref_mats, opaque, masked, view, proj, _, _), (_, mats, sel) = _soup(w, h, seed)
    depth, _ = D.depth_prepass(draws, view, proj, w, h, flags=D.QUANTIZE_D24, slots=[s for _, s in opaque])
    want = M.masked_pass(draws, view, proj, depth, w, h, materials=ref_mats, flags=G.QUANTIZE_D24, select=opaque, mask_select=masked)
    hotpath.raster_reserve(4096)
    try:
        got = run(hotpath, sel, mats, view, proj, depth, w, h, flags=G.QUANTIZE_D24)
    finally:
        hotpath.raster_reserve(0)
    same_masked(got, want, depth, f"D24 soup {w}x{h}")


def test_selection_kinds(hotpath):
    """Ranges are the other tests'. Visible lists in another order than the slots', with an index base: an ordinal is the position in its
    own selection's list, and the resolve finds the slot through keys64. Every slot as the masked selection beside an opaque list of
    nothing: a scene of masked models only, where the slots without bit 4 are never discarded."""
    w, h, seed = M.SOUPS[0]
    (draws, ref_mats, opaque, masked, view, proj, _, _), (dd, mats, _) = _soup(w, h, seed)
    n = len(draws)
    o_slots, m_slots = [s for _, s in opaque][::-1], [masked[k][1] for k in (3, 0, 5, 1, 4, 2)]
    depth, _ = D.depth_prepass(draws, view, proj, w, h, slots=o_slots)
    want = M.masked_pass(draws, view, proj, depth, w, h, materials=ref_mats, select=list(enumerate(o_slots)), mask_select=list(enumerate(m_slots)))
    got = run(hotpath, Selections(dd, o_slots, m_slots, "lists", index_base=1000), mats, view, proj, depth, w, h)
    same_masked(got, want, depth, "lists")
    assert want["won"] > 0 and (want["opaque_keys"] != 0).any()

    from unclerenderer_amd.hotpath import raster_draws
    sel = Selections(dd, [], [], "lists")
    sel.mask_draws = raster_draws(dd.commands)
    depth = np.zeros((h, w), np.float32)
    want = M.masked_pass(draws, view, proj, depth, w, h, materials=ref_mats, select=[], mask_select=[(k, k) for k in range(n)])
    got = run(hotpath, sel, mats, view, proj, depth, w, h)
    same_masked(got, want, depth, "every slot masked, no opaque draw")
    assert not want["opaque_keys"].any() and want["won"] == int((want["keys"] != 0).sum()) > 0


def _spanning_pair_scene(w, h):
    view, proj = D.soup_camera(w, h)
    inv = np.linalg.inv(view.astype(np.float64).reshape(4, 4))
    xs, ys = float(proj[0]), float(proj[5])
    rng = np.random.default_rng(5)

    def draw(pts, z, **kw):
        v = np.zeros((len(pts), 16), np.float32)
        pv = np.array([[(x / (0.5 * w) - 1.0) * z / xs, (1.0 - y / (0.5 * h)) * z / ys, z, 1.0] for x, y in pts])
        v[:, 0:3] = (pv @ inv)[:, :3]
        v[:, 3:6], v[:, 8:12] = (0, 0, -1), (1, 0, 0, 1)
        v[:, 6:8] = np.array(pts) / 16.0
        v[:, 12:16] = rng.uniform(0.5, 1.0, (len(pts), 4))
        return M.MaskDraw(v.reshape(-1).view(np.uint8).copy(), np.arange(len(pts), dtype=np.uint32), **kw)

    big = [(-3, -3), (-3, h + 3), (w + 3, -3), (w + 3, -3), (-3, h + 3), (w + 3, h + 3)]
    small = [p for x, y in rng.uniform(0, 100, (20, 2)) for p in ((x, y), (x, y + 9), (x + 9, y))]
    draws = [draw(big, 3.0, cutoff=0.3), draw(small, 1.0), draw(big, 2.0, cutoff=0.45)]
    mats = [{"key": 20, "base_color": X.random_texture(16, 16, 5, True, rng)}, {"key": 0}, {"key": 21, "base_color": X.random_texture(13, 7, 4, False, rng),
                                                                                             "normal": X.random_texture(8, 4, 1, False, rng)}]
    return draws, mats, view, proj


def test_masked_target_spanning_pairs(hotpath):
    """Two masked triangle pairs that span a 257 x 130 target, one behind the other, and 20 small opaque triangles in front: the
    large-triangle kernel runs the alpha test (with room in the queue), or the wave that found the triangle does (without)."""
    w, h = 257, 130
    draws, ref_mats, view, proj = _spanning_pair_scene(w, h)
    depth, _ = D.depth_prepass(draws, view, proj, w, h, slots=[1])
    want = M.masked_pass(draws, view, proj, depth, w, h, materials=ref_mats, select=[(1, 1)], mask_select=[(0, 0), (2, 2)])
    back, front = (want["keys"] >> 30 == 1).sum(), (want["keys"] >> 30 == 3).sum()
    assert back > 1000 and front > 1000 and (want["keys"] == 0).sum() > 100 and (want["clipped_in_front"] > 0).any()
    dd = device_draws(draws)
    sel, mats = Selections(dd, [1], [0, 2]), device_materials(ref_mats)
    try:
        for reserve in (1 << 12, 1, 0):
            hotpath.raster_reserve(reserve)
            got = run(hotpath, sel, mats, view, proj, depth, w, h)
            same_masked(got, want, depth, f"pairs, reserve {reserve}")
            assert (got["mask_stats"][3] == 0) if reserve == 1 << 12 else (got["mask_stats"][3] > 0), (reserve, got["mask_stats"].tolist())
    finally:
        hotpath.raster_reserve(0)


def test_no_materials_is_the_all_opaque_union(hotpath):
    """materials = NULL beside a mask: no slot has a key, nothing is discarded, and keys, targets and depth are DepthPrepass' and
    ur_gbuffer_pass' over the union of the two selections."""
    w, h, seed = M.SOUPS[0]
    (draws, _, opaque, masked, view, proj, depth, _), (dd, _, sel) = _soup(w, h, seed)
    got = run(hotpath, sel, None, view, proj, depth, w, h)
    want = M.masked_pass(draws, view, proj, depth, w, h, materials=None, select=opaque, mask_select=masked)
    same_masked(got, want, depth, "no materials")
    union_depth, _ = D.depth_prepass(draws, view, proj, w, h)
    union = G.gbuffer_pass(draws, view, proj, union_depth, w, h)
    assert np.array_equal(got["keys"], union["keys"]) and np.array_equal(got["depth"].view(np.uint32), union_depth.view(np.uint32))
    for k in ("A", "B", "C", "hdr"):
        assert np.array_equal(got[k], union[k]), k


def test_invalid_base_colour_descriptor_counts_as_clear(hotpath):
    """Key 20 with a descriptor that is broken each of the six ways: alpha is BaseColorAlpha * COLOR.a alone."""
    w, h, seed = M.SOUPS[0]
    (draws, ref_mats, opaque, masked, view, proj, depth, valid), (dd, _, sel) = _soup(w, h, seed)
    mats = [dict(m) for m in ref_mats]
    for (_, s), how in zip(masked, ("format", "null", "misaligned", "width", "height", "mips")):
        mats[s]["key"] = 20
        mats[s]["base_color"] = X.Tex(ref_mats[s]["base_color"].levels, True, False, how)
    want = M.masked_pass(draws, view, proj, depth, w, h, materials=mats, select=opaque, mask_select=masked)
    assert not any(layer["sampled"].any() for layer in want["layers"]) and not np.array_equal(want["keys"], valid["keys"])
    got = run(hotpath, sel, device_materials(mats), view, proj, depth, w, h)
    same_masked(got, want, depth, "invalid descriptors")


def test_parts_and_determinism(hotpath):
    """The raster part (six raster launches and the merge), then the resolve part, leave the one call's bytes; and a second run of the one
    call leaves the first one's."""
    from unclerenderer_amd import lib
    w, h, seed = M.SOUPS[1]
    (_, _, _, _, view, proj, depth, want), (_, mats, sel) = _soup(w, h, seed)
    hotpath.raster_reserve(4096)
    try:
        first = run(hotpath, sel, mats, view, proj, depth, w, h)
        second = run(hotpath, sel, mats, view, proj, depth, w, h)
        apart = run(hotpath, sel, mats, view, proj, depth, w, h, parts_sequence=(lib.UR_GBUFFER_PART_RASTER, lib.UR_GBUFFER_PART_RESOLVE))
        raster_only = run(hotpath, sel, mats, view, proj, depth, w, h, parts_sequence=(lib.UR_GBUFFER_PART_RASTER,))
    finally:
        hotpath.raster_reserve(0)
    same_masked(first, want, depth, "one call")
    same_masked(apart, want, depth, "raster part, then resolve part")
    assert first["won"] == second["won"]
    for k in ("keys", "keys64", "A", "B", "C", "hdr"):
        assert np.array_equal(first[k], second[k]), k
    assert np.array_equal(first["depth"].view(np.uint32), second["depth"].view(np.uint32))
    assert np.array_equal(raster_only["keys"], want["keys"]) and (raster_only["C"] == 0x5A5A5A5A).all() and np.isnan(raster_only["A"].view(np.float16)).all()


def test_null_mask_is_ur_gbuffer_pass_materials(hotpath, urlib):
    """mask == NULL: ur_gbuffer_pass_materials' bytes, and depth is not written."""
    import ctypes as C

    import torch
    from unclerenderer_amd import lib
    from unclerenderer_amd.hotpath import gbuffer_targets, raster_draws
    from tests.gbuffer_gpu import same
    w, h, seed = M.SOUPS[0]
    (draws, ref_mats, _, _, view, proj, _, _), (dd, mats, _) = _soup(w, h, seed)
    depth, _ = D.depth_prepass(draws, view, proj, w, h)
    want = X.gbuffer_pass(draws, view, proj, depth, w, h, materials=ref_mats)
    dev_depth = torch.from_numpy(depth.copy()).to("cuda")
    half = lambda: torch.full((h, w, 4), float("nan"), dtype=torch.float16, device="cuda")  # noqa: E731
    word = lambda: torch.full((h, w), 0x5A5A5A5A, dtype=torch.int32, device="cuda")  # noqa: E731
    a, b, hdr, c, keys = half(), half(), half(), word(), word()
    stats = torch.zeros(6, dtype=torch.int32, device="cuda")
    tg, d = gbuffer_targets(a, b, c, hdr, keys), raster_draws(dd.commands)
    v, p = (np.ascontiguousarray(m, np.float32).reshape(-1) for m in (view, proj))
    rc = urlib.ur_gbuffer_pass_masked(hotpath._ctx, lib.fptr(v), lib.fptr(p), C.byref(d), C.c_void_p(dev_depth.data_ptr()), C.byref(tg), w, h, 0, h, 0, 0,
                                      C.c_void_p(stats.data_ptr()), C.c_void_p(mats.table.data_ptr()), mats.count, None)
    assert rc == lib.UR_OK
    torch.cuda.synchronize()
    got = {"A": a.cpu().numpy().view(np.uint16), "B": b.cpu().numpy().view(np.uint16), "hdr": hdr.cpu().numpy().view(np.uint16),
           "C": c.cpu().numpy().view(np.uint32), "keys": keys.cpu().numpy().view(np.uint32), "stats": stats.cpu().numpy().view(np.uint32)}
    same(got, want, "mask == NULL")
    assert np.array_equal(dev_depth.cpu().numpy().view(np.uint32), depth.view(np.uint32))
