"""ur_gbuffer_pass_materials on the GPU: keys, A, B, C, HDR, ObjectId and stats6 (except [3], structural) are byte-equal to
tests/gbuffer_tex_ref.py, the rule of DESIGN.md section 3.10; NaN is compared by NaN-ness."""
import numpy as np
import pytest

from tests import depth_ref as D
from tests import gbuffer_ref as G
from tests import gbuffer_tex_ref as X
from tests.gbuffer_gpu import device_draws, run, same
from tests.gbuffer_tex_gpu import device_materials
from tests.test_gbuffer_tex_ref import H as HAND_H
from tests.test_gbuffer_tex_ref import W as HAND_W
from tests.test_gbuffer_tex_ref import edge_soup_reference, hand_cases, soup_reference

pytestmark = pytest.mark.gpu


def _depth(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to("cuda")


@pytest.mark.parametrize("flags", [0, G.QUANTIZE_D24])
@pytest.mark.parametrize("name", sorted(hand_cases()))
def test_hand_cases(hotpath, name, flags):
    draws, mats = hand_cases()[name]
    cam = D.hand_camera(HAND_W, HAND_H)
    depth, _ = D.depth_prepass(draws, *cam, HAND_W, HAND_H, flags=flags)
    want = X.gbuffer_pass(draws, *cam, depth, HAND_W, HAND_H, materials=mats, flags=flags)
    got = run(hotpath, device_draws(draws), *cam, _depth(depth), HAND_W, HAND_H, flags=flags, materials=device_materials(mats))
    same(got, want, name)


@pytest.mark.parametrize("w,h,seed", X.SOUPS)
def test_soups(hotpath, w, h, seed):
    """A material per draw cycling through keys 0-15; with the queue, with a queue of one entry and without one; with and without the
    ObjectId output; the band [37, 78) of 257 x 130 (an odd row0: the quads stay anchored at even frame rows) against the same rows of
    the whole."""
    draws, view, proj, depth, want = soup_reference(w, h, seed)
    dd, dm, dev_depth = device_draws(draws), device_materials(X.soup_materials(seed)), _depth(depth)
    try:
        for reserve in (1 << 16, 1, 0):
            hotpath.raster_reserve(reserve)
            for oid in (True, False):  # both instantiations of the textured resolve
                got = run(hotpath, dd, view, proj, dev_depth, w, h, object_id=oid, materials=dm)
                same(got, want, f"soup {w}x{h}, reserve {reserve}, ObjectId {oid}")
                if h > 78:
                    band = run(hotpath, dd, view, proj, dev_depth, w, h, 37, 41, object_id=oid, materials=dm)
                    same(band, want, f"soup {w}x{h} rows [37, 78), reserve {reserve}, ObjectId {oid}", 37, 41)
    finally:
        hotpath.raster_reserve(0)


def test_edge_shape_soup(hotpath):
    """The 64 x 64 soup under textures at the ends of ur_texture2d's ranges (gbuffer_tex_ref.EDGE_SHAPES: 65535 texels each way, chains of
    16 and 17 levels, sizes that are no power of two, 8 MB at level 0), with a 65536-entry queue and without one, ObjectId on."""
    w, h, _ = X.SOUPS[0]
    draws, view, proj, depth, mats, want = edge_soup_reference()
    dd, dm, dev_depth = device_draws(draws), device_materials(mats), _depth(depth)
    try:
        for reserve in (1 << 16, 0):
            hotpath.raster_reserve(reserve)
            got = run(hotpath, dd, view, proj, dev_depth, w, h, materials=dm)
            same(got, want, f"edge shapes, reserve {reserve}")
    finally:
        hotpath.raster_reserve(0)


class _NoCommands:
    commands = None


def test_selections_short_table_invalid_descriptor_and_zero_keys(hotpath):
    """Every slot, a list with an index base (the material follows the slot, not the ordinal), ranges; a table shorter than the command
    count; an invalid descriptor under a set bit; an all-zero-key table against ur_gbuffer_pass."""
    import torch
    from unclerenderer_amd.hotpath import to_device
    w, h, seed = X.SOUPS[0]
    draws, view, proj, _, _ = soup_reference(w, h, seed)
    n = len(draws)
    dd = device_draws(draws)
    mats = X.soup_materials(seed)

    def check(select, what, mats_=mats, dd_=dd, **kw):
        slots = None if select is None else [s for _, s in select]
        depth, _ = D.depth_prepass(draws, view, proj, w, h, slots=slots)
        want = X.gbuffer_pass(draws, view, proj, depth, w, h, materials=mats_, select=select)
        got = run(hotpath, dd_, view, proj, _depth(depth), w, h, materials=device_materials(mats_), **kw)
        same(got, want, what)
        return got

    base = 1000
    idx = np.array([base + 15, base + 7, base + 3, base + 11, base + 5], np.uint32)
    select = G.selection(n, visible=(idx, 4), index_base=base)
    assert select == [(0, 15), (1, 7), (2, 3), (3, 11)]
    check(select, "list of 4", visible=(to_device(idx), to_device(np.array([4], np.uint32))), index_base=base)
    offsets, counts = np.array([0, 6, 6, 18], np.uint32), np.array([4, 0, 9], np.uint32)
    select = G.selection(n, ranges=(offsets, counts))
    assert [s for _, s in select] == [0, 1, 2, 3] + list(range(6, 15))
    compacted = torch.from_numpy(dd.host_commands.view(np.int32).copy()).to("cuda")
    check(select, "ranges", dd_=_NoCommands(), ranges=(to_device(offsets), compacted, to_device(counts)))
    check(None, "material_count 7 of 18", mats[:7])
    broken = [dict(m) for m in mats]
    ways = ("format", "null", "misaligned", "width", "height", "mips")  # every branch of the descriptor check, each under a set bit, all four maps
    for j, (k, how) in enumerate(zip((15, 7, 11, 13, 14, 6), ways)):
        name, bit, _ = X.MAPS[j % 4]
        assert mats[k]["key"] & bit
        broken[k][name] = X.Tex(broken[k][name].levels, broken[k][name].srgb, valid=False, how=how)
    check(None, "invalid descriptors", broken)
    zero = check(None, "all keys zero", [dict(m, key=0) for m in mats])
    depth, _ = D.depth_prepass(draws, view, proj, w, h)
    plain = run(hotpath, dd, view, proj, _depth(depth), w, h)
    for k in ("A", "B", "C", "hdr", "keys", "object_id"):
        assert np.array_equal(zero[k], plain[k]), k


def test_parts(hotpath):
    """ur_gbuffer_pass_materials_parts: the raster part, then the resolve part, leave ur_gbuffer_pass_materials' bytes."""
    import torch
    from unclerenderer_amd import lib
    from unclerenderer_amd.hotpath import gbuffer_targets
    w, h, seed = X.SOUPS[0]
    draws, view, proj, depth, want = soup_reference(w, h, seed)
    dd, dm, dev_depth = device_draws(draws), device_materials(X.soup_materials(seed)), _depth(depth)
    half = lambda: torch.full((h, w, 4), float("nan"), dtype=torch.float16, device="cuda")  # noqa: E731
    word = lambda: torch.full((h, w), 0x5A5A5A5A, dtype=torch.int32, device="cuda")  # noqa: E731
    a, b, hdr, c, keys, oid = half(), half(), half(), word(), word(), word()
    stats = torch.zeros(6, dtype=torch.int32, device="cuda")
    tg = gbuffer_targets(a, b, c, hdr, keys, oid)
    hotpath.gbuffer_pass(view, proj, dd.commands, dev_depth, tg, w, h, stats=stats, parts=lib.UR_GBUFFER_PART_RASTER, materials=dm)
    torch.cuda.synchronize()
    assert np.array_equal(keys.cpu().numpy().view(np.uint32), want["keys"])
    assert all(bool(torch.isnan(t).all()) for t in (a, b, hdr)) and all(bool((t == 0x5A5A5A5A).all()) for t in (c, oid))
    counted = stats.cpu().numpy().copy()
    hotpath.gbuffer_pass(view, proj, dd.commands, dev_depth, tg, w, h, stats=stats, parts=lib.UR_GBUFFER_PART_RESOLVE, materials=dm)
    torch.cuda.synchronize()
    assert np.array_equal(stats.cpu().numpy(), counted)
    got = {"A": a, "B": b, "hdr": hdr, "C": c, "keys": keys, "object_id": oid}
    got = {k: t.cpu().numpy().view(np.uint16 if t.dtype == torch.float16 else np.uint32) for k, t in got.items()}
    got["stats"] = counted.view(np.uint32)
    same(got, want, "raster part, then resolve part")
