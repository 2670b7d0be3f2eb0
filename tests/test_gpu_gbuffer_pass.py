"""ur_gbuffer_pass on the GPU: keys, A, B, C, HDR, ObjectId and stats6 (except [3], structural) are byte-equal to tests/gbuffer_ref.py,
the rule of DESIGN.md section 3.9; NaN is compared by NaN-ness."""
import numpy as np
import pytest

from tests import depth_ref as D
from tests import gbuffer_ref as G
from tests.gbuffer_gpu import device_draws, run, same
from tests.test_gbuffer_ref import H as HAND_H
from tests.test_gbuffer_ref import W as HAND_W
from tests.test_gbuffer_ref import hand_cases, soup_reference

pytestmark = pytest.mark.gpu


def _depth(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to("cuda")


@pytest.mark.parametrize("flags", [0, G.QUANTIZE_D24])
@pytest.mark.parametrize("name", sorted(hand_cases()))
def test_hand_cases(hotpath, name, flags):
    draws = hand_cases()[name]
    cam = D.hand_camera(HAND_W, HAND_H)
    depth, _ = D.depth_prepass(draws, *cam, HAND_W, HAND_H, flags=flags)
    want = G.gbuffer_pass(draws, *cam, depth, HAND_W, HAND_H, flags=flags)
    got = run(hotpath, device_draws(draws), *cam, _depth(depth), HAND_W, HAND_H, flags=flags)
    same(got, want, name)


@pytest.mark.parametrize("w,h,seed", G.SOUPS)
def test_soups(hotpath, w, h, seed):
    """With the queue, with a queue of one entry and without one; with and without the ObjectId output; the band [37, 78) of 257 x 130
    against the same rows of the whole; the depth from ur_depth_prepass in the same stream."""
    import torch
    draws, view, proj, depth, want = soup_reference(w, h, seed)
    dd = device_draws(draws)
    dev_depth = torch.full((h, w), float("nan"), dtype=torch.float32, device="cuda")
    try:
        for reserve in (1 << 16, 1, 0):
            hotpath.raster_reserve(reserve)
            hotpath.depth_prepass(view, proj, dd.commands, dev_depth)  # same stream, no synchronisation in between
            got = run(hotpath, dd, view, proj, dev_depth, w, h, object_id=reserve != 1)
            assert np.array_equal(dev_depth.cpu().numpy().view(np.uint32), depth.view(np.uint32))
            same(got, want, f"soup {w}x{h}, reserve {reserve}")
            if h > 78:
                band = run(hotpath, dd, view, proj, dev_depth, w, h, 37, 41)
                same(band, want, f"soup {w}x{h} rows [37, 78), reserve {reserve}", 37, 41)
    finally:
        hotpath.raster_reserve(0)


@pytest.mark.parametrize("w,h,seed", G.SOUPS)
def test_soups_d24(hotpath, w, h, seed):
    draws, view, proj, _, _ = soup_reference(w, h, seed)
    depth, _ = D.depth_prepass(draws, view, proj, w, h, flags=D.QUANTIZE_D24)
    want = G.gbuffer_pass(draws, view, proj, depth, w, h, flags=G.QUANTIZE_D24)
    hotpath.raster_reserve(4096)
    try:
        got = run(hotpath, device_draws(draws), view, proj, _depth(depth), w, h, flags=G.QUANTIZE_D24)
    finally:
        hotpath.raster_reserve(0)
    same(got, want, f"D24 soup {w}x{h}")


class _NoCommands:
    commands = None


def test_selections(hotpath):
    """All slots, a list with an index base (the ordinal is the position in the list: another draw order), ranges."""
    import torch
    from unclerenderer_amd.hotpath import to_device
    w, h = 64, 64
    draws = G.soup(w, h, 7, triangles=600)
    draws[1].instance_count = 1
    n = len(draws)
    dd = device_draws(draws)
    view, proj = D.soup_camera(w, h)

    def check(select, what, dd_=dd, **kw):
        slots = None if select is None else [s for _, s in select]
        depth, _ = D.depth_prepass(draws, view, proj, w, h, slots=slots)
        want = G.gbuffer_pass(draws, view, proj, depth, w, h, select=select)
        got = run(hotpath, dd_, view, proj, _depth(depth), w, h, **kw)
        same(got, want, what)
        return want

    every = check(None, "every slot")
    base = 1000
    idx = np.array([base + 4, base + 0, base + 2, base + 1, base + 3], np.uint32)
    for count in (3, 0):
        select = G.selection(n, visible=(idx, count), index_base=base)
        assert select == [(0, 4), (1, 0), (2, 2)][:count]
        listed = check(select, f"list of {count}", visible=(to_device(idx), to_device(np.array([count], np.uint32))), index_base=base)
        if count == 0:
            assert not listed["keys"].any()
        else:
            assert set((listed["keys"][listed["keys"] != 0] >> G.key_bits(n)).tolist()) == {1, 2, 3}
    offsets, counts = np.array([0, 2, 2, 5], np.uint32), np.array([1, 0, 3], np.uint32)
    select = G.selection(n, ranges=(offsets, counts))
    assert select == [(0, 0), (2, 2), (3, 3), (4, 4)]
    compacted = torch.from_numpy(dd.host_commands.view(np.int32).copy()).to("cuda")
    check(select, "ranges", _NoCommands(), ranges=(to_device(offsets), compacted, to_device(counts)))
    assert every["keys"].any()


def test_target_spanning_pair_and_key_bits(hotpath):
    """Two triangles that span a 257 x 130 target (large: the queue's record carries the key) beside a command of 20 small ones: with
    key_triangle_bits = 4 the command of 20 is counted in stats[1] and not drawn, the others are unaffected."""
    w, h = 257, 130
    view, proj = D.soup_camera(w, h)
    inv = np.linalg.inv(view.astype(np.float64).reshape(4, 4))
    xs, ys = float(proj[0]), float(proj[5])

    def world(pts, z):
        pv = np.array([[(x / (0.5 * w) - 1.0) * z / xs, (1.0 - y / (0.5 * h)) * z / ys, z, 1.0] for x, y in pts])
        return (pv @ inv)[:, :3].astype(np.float32)

    big = world([(-3, -3), (-3, h + 3), (w + 3, -3), (w + 3, -3), (-3, h + 3), (w + 3, h + 3)], 2.0)
    rng = np.random.default_rng(5)
    small = np.concatenate([world([(x, y), (x, y + 9), (x + 9, y)], 1.0) for x, y in rng.uniform(0, 100, (20, 2))])
    mk = lambda p, oid: G.GDraw(G.vertex_buffer(p, colors=rng.uniform(0, 1, (p.shape[0], 3))), np.arange(p.shape[0], dtype=np.uint32), object_id=oid)  # noqa: E731
    draws = [mk(big, 11), mk(small, 22), mk(big, 33)]
    dd = device_draws(draws)
    try:
        for bits in (0, 4):
            # (the caller's ranges keep a command the pass cannot draw out of the prepass too: its depth would hide what lies behind it)
            depth, _ = D.depth_prepass(draws, view, proj, w, h, slots=[0, 2] if bits else None)
            want = G.gbuffer_pass(draws, view, proj, depth, w, h, key_triangle_bits=bits)
            assert want["stats"][1] == (20 if bits else 0) and (want["keys"] != 0).all()
            assert set(want["object_id"].reshape(-1).tolist()) == ({33} if bits else {22, 33})
            for reserve in (1 << 12, 1, 0):
                hotpath.raster_reserve(reserve)
                got = run(hotpath, dd, view, proj, _depth(depth), w, h, key_triangle_bits=bits)
                same(got, want, f"pair, bits {bits}, reserve {reserve}")
                assert (got["stats"][3] == 0) if reserve == 1 << 12 else (got["stats"][3] > 0), (reserve, got["stats"].tolist())
    finally:
        hotpath.raster_reserve(0)


def test_parts(hotpath):
    """ur_gbuffer_pass_parts: the raster part writes the keys and the counters and nothing else, the resolve part over them the other
    targets and no counter; together they leave ur_gbuffer_pass' bytes."""
    import torch
    from unclerenderer_amd import lib
    from unclerenderer_amd.hotpath import gbuffer_targets
    w, h, seed = G.SOUPS[0]
    draws, view, proj, depth, want = soup_reference(w, h, seed)
    dd, dev_depth = device_draws(draws), _depth(depth)
    half = lambda: torch.full((h, w, 4), float("nan"), dtype=torch.float16, device="cuda")  # noqa: E731
    word = lambda: torch.full((h, w), 0x5A5A5A5A, dtype=torch.int32, device="cuda")  # noqa: E731
    a, b, hdr, c, keys, oid = half(), half(), half(), word(), word(), word()
    stats = torch.zeros(6, dtype=torch.int32, device="cuda")
    tg = gbuffer_targets(a, b, c, hdr, keys, oid)
    hotpath.gbuffer_pass(view, proj, dd.commands, dev_depth, tg, w, h, stats=stats, parts=lib.UR_GBUFFER_PART_RASTER)
    torch.cuda.synchronize()
    assert np.array_equal(keys.cpu().numpy().view(np.uint32), want["keys"])
    assert all(bool(torch.isnan(t).all()) for t in (a, b, hdr)) and all(bool((t == 0x5A5A5A5A).all()) for t in (c, oid))
    counted = stats.cpu().numpy().copy()
    hotpath.gbuffer_pass(view, proj, dd.commands, dev_depth, tg, w, h, stats=stats, parts=lib.UR_GBUFFER_PART_RESOLVE)
    torch.cuda.synchronize()
    assert np.array_equal(stats.cpu().numpy(), counted)
    got = {"A": a, "B": b, "hdr": hdr, "C": c, "keys": keys, "object_id": oid}
    got = {k: t.cpu().numpy().view(np.uint16 if t.dtype == torch.float16 else np.uint32) for k, t in got.items()}
    got["stats"] = counted.view(np.uint32)
    same(got, want, "raster part, then resolve part")
