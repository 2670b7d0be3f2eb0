"""ur_object_id_pass and ur_object_id_pick on the GPU: keys, ObjectId, the pick's records and stats6 (except [3], structural) are byte-equal
to tests/object_id_ref.py, the rule of DESIGN.md section 3.16, and to ur_gbuffer_pass' optional ObjectId output, the earlier way to the same
picture; the float64 ray casters hold the ids independently (tests/object_id_raycast.py)."""
import numpy as np
import pytest

from tests import depth_ref as D
from tests import forward_ref as FW
from tests import gbuffer_mask_gpu
from tests import gbuffer_ref as G
from tests import object_id_raycast as OR
from tests import object_id_ref as O
from tests import raycast_ref as R
from tests import raycast_tex as T
from tests import test_object_id_ref as TO
from tests.forward_gpu import DeviceFrame
from tests.forward_gpu import run as run_forward
from tests.gbuffer_gpu import device_draws
from tests.gbuffer_gpu import run as run_gbuffer
from tests.gbuffer_tex_gpu import device_materials
from tests.test_gbuffer_mask_ref import soup_reference as masked_soup_reference
from tests.test_gbuffer_ref import soup_reference

pytestmark = pytest.mark.gpu

COUNTED = [0, 1, 2, 4, 5]  # stats6 without the structural [3]
POISON = 0x5A5A5A5A


def _device(a, dtype=np.float32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype).copy()).to("cuda")


def every_slot(dd):
    from unclerenderer_amd.hotpath import raster_draws
    sel = raster_draws(dd.commands)
    sel._keep.append(dd)  # (the commands point into dd's buffers)
    return sel


def run_image(hotpath, sel, view, proj, depth, w, h, row0=0, rows=None, **kw):
    """ur_object_id_pass over poisoned band targets and zeroed stats: {keys, object_id (the band's rows), stats}. depth: (h, w) float32, on
    the host or the device."""
    import torch
    rows = h - row0 if rows is None else rows
    depth = depth if isinstance(depth, torch.Tensor) else _device(depth)
    oid = torch.full((rows, w), POISON, dtype=torch.int32, device="cuda")
    keys = torch.full((rows, w), POISON, dtype=torch.int32, device="cuda")
    stats = torch.zeros(6, dtype=torch.int32, device="cuda")
    hotpath.object_id_pass(sel, view, proj, depth, w, h, object_id=oid, keys=keys, row0=row0, rows=rows, stats=stats, **kw)
    torch.cuda.synchronize()
    return {k: t.cpu().numpy().view(np.uint32) for k, t in (("keys", keys), ("object_id", oid), ("stats", stats))}


def run_pick(hotpath, sel, view, proj, depth, w, h, points, **kw):
    """ur_object_id_pick over poisoned records and stats of 100 each: ((n, 4) uint32 records, what the call added to stats6)."""
    import torch
    depth = depth if isinstance(depth, torch.Tensor) else _device(depth)
    records = torch.full((len(points), 4), POISON, dtype=torch.int32, device="cuda")
    stats = torch.full((6,), 100, dtype=torch.int32, device="cuda")
    got = hotpath.object_id_pick(sel, view, proj, depth, w, h, points, results=records, stats=stats, **kw)
    torch.cuda.synchronize()
    assert got is records
    return records.cpu().numpy().view(np.uint32), stats.cpu().numpy().view(np.uint32) - np.uint32(100)


def same_image(got, want, what, row0=0, rows=None):
    band = slice(row0, None if rows is None else row0 + rows)
    for k in ("keys", "object_id"):
        bad = got[k] != want[k][band]
        assert not bad.any(), f"{what}: {k}: {int(bad.sum())} texels differ, first at {tuple(int(v) for v in np.argwhere(bad)[0])}"
    assert got["stats"][COUNTED].tolist() == want["stats"][COUNTED].tolist(), (what, got["stats"].tolist(), want["stats"].tolist())


def same_pick(got, want_image, points, w, h, what):
    records, added = got
    want = O.pick(want_image, points, w, h)
    bad = (records != want).any(axis=1)
    assert not bad.any(), f"{what}: {int(bad.sum())} records differ, first: point {points[int(np.argmax(bad))]} got {records[np.argmax(bad)].tolist()}, want {want[np.argmax(bad)].tolist()}"
    assert added[3] == 0 and added[COUNTED].tolist() == want_image["stats"][COUNTED].tolist(), (what, added.tolist(), want_image["stats"].tolist())


def mixed_points(w, h, seed, covered=None):
    """64 points of a w x h frame: the four corners, three out of range (they clamp), a duplicate, and seeded ones - from `covered` texels
    (a boolean image) for half of them when given."""
    rng = np.random.default_rng(seed)
    pts = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w, 5), (7, 0xFFFFFFFF), (0x80000000, h + 100)]
    if covered is not None and covered.any():
        ys, xs = np.nonzero(covered)
        pick = rng.integers(0, ys.size, 28)
        pts += [(int(xs[k]), int(ys[k])) for k in pick]
    while len(pts) < 63:
        pts.append((int(rng.integers(w)), int(rng.integers(h))))
    return pts + [pts[9]]


# ---- the hand-worked 8 x 8 answers -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", [0, G.QUANTIZE_D24])
@pytest.mark.parametrize("name", sorted(TO.hand_cases()))
def test_hand_cases(hotpath, name, flags):
    case = TO.hand_cases()[name]
    cam = D.hand_camera(TO.W, TO.H)
    depth = TO.case_depth(case, flags)
    want = O.image(case[0], *cam, depth, TO.W, TO.H, flags=flags)
    sel = every_slot(device_draws(case[0]))
    same_image(run_image(hotpath, sel, *cam, depth, TO.W, TO.H, flags=flags), want, name)
    (points,) = O.every_texel(TO.W, TO.H)
    same_pick(run_pick(hotpath, sel, *cam, depth, TO.W, TO.H, points, flags=flags), want, points, TO.W, TO.H, name)
    clamped = [(TO.W, 0xFFFFFFFF), (0xFFFFFFFF, 0), (TO.W + 1, TO.H + 1)]
    same_pick(run_pick(hotpath, sel, *cam, depth, TO.W, TO.H, clamped, flags=flags), want, clamped, TO.W, TO.H, f"{name}, clamped points")


# ---- the image pass ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", [0, G.QUANTIZE_D24])
@pytest.mark.parametrize("w,h,seed", G.SOUPS)
def test_soups_against_the_restatement_and_the_old_entry_point(hotpath, w, h, seed, flags):
    """Under the prepass' own depth and under one it never wrote (a texel's depth above every fragment, or below several of them): the
    restatement's bytes, ur_gbuffer_pass(..., object_id=...)'s keys and object_id, and the same bytes from a second run."""
    draws, view, proj, depth, _ = soup_reference(w, h, seed)
    if flags:
        depth, _ = D.depth_prepass(draws, view, proj, w, h, flags=flags)
    rng = np.random.default_rng(seed + 50)
    other = np.where(rng.uniform(size=(h, w)) < 0.5, depth, rng.uniform(0.0, 0.2, (h, w))).astype(np.float32)
    dd = device_draws(draws)
    sel = every_slot(dd)
    for name, dep in (("own depth", depth), ("another depth", other)):
        want = O.image(draws, view, proj, dep, w, h, flags=flags)
        dev = _device(dep)
        got = run_image(hotpath, sel, view, proj, dev, w, h, flags=flags)
        same_image(got, want, f"soup {w}x{h} flags {flags}, {name}")
        old = run_gbuffer(hotpath, dd, view, proj, dev, w, h, flags=flags)
        assert np.array_equal(got["keys"], old["keys"]) and np.array_equal(got["object_id"], old["object_id"]) and got["stats"].tolist() == old["stats"].tolist()
        again = run_image(hotpath, sel, view, proj, dev, w, h, flags=flags)
        assert all(np.array_equal(again[k], got[k]) for k in got)
        assert np.array_equal(dev.cpu().numpy().view(np.uint32), dep.view(np.uint32)), "depth was written"
    assert (want["keys"] == 0).any() and (want["keys"] != 0).any()


class _Selections:
    """Every slot, a visible list with an index base (the ordinal is the position in the list: another draw order) and ranges over one soup,
    as (name, gbuffer_ref.selection list, ur_raster_draws)."""

    def __init__(self, draws, dd):
        import torch
        from unclerenderer_amd.hotpath import raster_draws, to_device
        self.dd = dd  # (the commands point into its buffers)
        n, base = len(draws), 1000
        idx = np.array([base + 4, base + 0, base + 2, base + 1, base + 3], np.uint32)
        offsets, counts = np.array([0, 2, 2, 5], np.uint32), np.array([1, 0, 3], np.uint32)
        compacted = torch.from_numpy(dd.host_commands.view(np.int32).copy()).to("cuda")
        self.all = [("every slot", None, raster_draws(dd.commands)),
                    ("list of 3", G.selection(n, visible=(idx, 3), index_base=base), raster_draws(dd.commands, None, (to_device(idx), to_device(np.array([3], np.uint32))), None, base)),
                    ("ranges", G.selection(n, ranges=(offsets, counts)), raster_draws(None, None, None, (to_device(offsets), compacted, to_device(counts))))]
        assert self.all[1][1] == [(0, 4), (1, 0), (2, 2)] and self.all[2][1] == [(0, 0), (2, 2), (3, 3), (4, 4)]


def test_selections(hotpath):
    """The image and the pick under every slot, a list and ranges; a point_count of 1 and of 64."""
    w, h = 64, 64
    draws = G.soup(w, h, 7, triangles=600)
    draws[1].instance_count = 1
    view, proj = D.soup_camera(w, h)
    selections = _Selections(draws, device_draws(draws))
    for name, select, sel in selections.all:
        depth, _ = D.depth_prepass(draws, view, proj, w, h, slots=None if select is None else [s for _, s in select])
        want = O.image(draws, view, proj, depth, w, h, select=select)
        assert want["keys"].any()
        same_image(run_image(hotpath, sel, view, proj, depth, w, h), want, name)
        points = mixed_points(w, h, 3, want["keys"] != 0)
        same_pick(run_pick(hotpath, sel, view, proj, depth, w, h, points), want, points, w, h, f"{name}, 64 points")
        same_pick(run_pick(hotpath, sel, view, proj, depth, w, h, points[20:21]), want, points[20:21], w, h, f"{name}, 1 point")


def test_target_spanning_pair_with_and_without_the_queue(hotpath):
    """tests/test_gpu_gbuffer_pass.py's pair: two triangles that span a 257 x 130 target, twice, beside a command of 20 small ones; through
    the large-triangle queue, a queue of one entry and none. The pick has no queue: it never adds to stats6[3]."""
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
    sel = every_slot(device_draws(draws))
    depth, _ = D.depth_prepass(draws, view, proj, w, h)
    want = O.image(draws, view, proj, depth, w, h)
    assert set(want["object_id"].reshape(-1).tolist()) == {22, 33}
    points = mixed_points(w, h, 8)
    try:
        for reserve in (1 << 12, 1, 0):
            hotpath.raster_reserve(reserve)
            got = run_image(hotpath, sel, view, proj, depth, w, h)
            same_image(got, want, f"pair, reserve {reserve}")
            assert (got["stats"][3] == 0) if reserve == 1 << 12 else (got["stats"][3] > 0), (reserve, got["stats"].tolist())
            same_pick(run_pick(hotpath, sel, view, proj, depth, w, h, points), want, points, w, h, f"pair, reserve {reserve}")
    finally:
        hotpath.raster_reserve(0)


@pytest.mark.parametrize("bands", [[(0, 65), (65, 65)], [(0, 37), (37, 41), (78, 52)]])
def test_bands_against_the_whole_frame(hotpath, bands):
    w, h, seed = G.SOUPS[1]
    draws, view, proj, depth, _ = soup_reference(w, h, seed)
    sel = every_slot(device_draws(draws))
    dev = _device(depth)
    whole = run_image(hotpath, sel, view, proj, dev, w, h)
    same_image(whole, O.image(draws, view, proj, depth, w, h), "the whole frame")
    for row0, rows in bands:
        got = run_image(hotpath, sel, view, proj, dev, w, h, row0, rows)
        same_image(got, whole, f"rows [{row0}, {row0 + rows})", row0, rows)  # (triangles are counted whether or not they touch the band)


@pytest.mark.parametrize("w,h,seed", G.SOUPS)
def test_on_the_depth_the_masked_and_the_forward_pass_raise(hotpath, w, h, seed):
    """The masked soup: ur_gbuffer_pass_masked and ur_forward_pass each raise a copy of the opaque prepass' depth; ur_object_id_pass over the
    union of both selections against either is the restatement's image against the restated raised depth, and so is the pick."""
    draws, mats, opaque, masked, view, proj, depth, ref = masked_soup_reference(w, h, seed)
    dd = device_draws(draws)
    dmats = device_materials(mats)
    msel = gbuffer_mask_gpu.Selections(dd, [s for _, s in opaque], [s for _, s in masked])
    raised_g = gbuffer_mask_gpu.run(hotpath, msel, dmats, view, proj, depth, w, h)["depth"]
    raised_f = run_forward(hotpath, msel, dmats, view, proj, depth, w, h, DeviceFrame(hotpath, FW.soup_frame(w, h, seed)), T.background(w, h))["depth"]
    assert np.array_equal(raised_g.view(np.uint32), ref["depth"].view(np.uint32)) and np.array_equal(raised_f.view(np.uint32), raised_g.view(np.uint32))
    want = O.image(draws, view, proj, ref["depth"], w, h)
    sel = every_slot(dd)
    got_g, got_f = (run_image(hotpath, sel, view, proj, dep, w, h) for dep in (raised_g, raised_f))
    same_image(got_g, want, f"masked soup {w}x{h}, the masked pass' depth")
    same_image(got_f, want, f"masked soup {w}x{h}, the forward pass' depth")
    assert all(np.array_equal(got_g[k], got_f[k]) for k in got_g)
    # the quirk is there to be seen: texels whose ObjectId is not the G-buffer's winning draw
    gslot = np.where(ref["keys"] != 0, (ref["keys"] >> G.key_bits(len(draws))).astype(np.int64) - 1, -1)
    assert ((want["slot"].astype(np.int64) != gslot) & (want["keys"] != 0) & (gslot >= 0)).any()
    points = mixed_points(w, h, seed, want["slot"].astype(np.int64) != np.where(gslot >= 0, gslot, O.NO_SLOT))
    same_pick(run_pick(hotpath, sel, view, proj, raised_g, w, h, points), want, points, w, h, f"masked soup {w}x{h}, pick")


# ---- the pick -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", [0, G.QUANTIZE_D24])
def test_pick_at_every_texel_of_64_x_64(hotpath, flags):
    """64 calls of 64 points: the image's keys and ObjectId, and the restatement's records, at every texel."""
    import torch
    w, h, seed = G.SOUPS[0]
    draws, view, proj, depth, _ = soup_reference(w, h, seed)
    if flags:
        depth, _ = D.depth_prepass(draws, view, proj, w, h, flags=flags)
    want = O.image(draws, view, proj, depth, w, h, flags=flags)
    sel = every_slot(device_draws(draws))
    dev = _device(depth)
    image = run_image(hotpath, sel, view, proj, dev, w, h, flags=flags)
    calls = O.every_texel(w, h)
    assert len(calls) == 64 and all(len(c) == 64 for c in calls)
    records = torch.full((len(calls), 64, 4), POISON, dtype=torch.int32, device="cuda")
    stats = torch.zeros(6, dtype=torch.int32, device="cuda")
    for k, points in enumerate(calls):  # (asynchronous: nothing is read back between the calls)
        hotpath.object_id_pick(sel, view, proj, dev, w, h, points, results=records[k], flags=flags, stats=stats)
    torch.cuda.synchronize()
    got = records.cpu().numpy().view(np.uint32).reshape(h, w, 4)
    assert np.array_equal(got[..., 0], image["object_id"]) and np.array_equal(got[..., 1], image["keys"])
    for k, name in enumerate(("object_id", "keys", "slot", "depth_bits")):
        assert np.array_equal(got[..., k], want[name]), name
    added = stats.cpu().numpy().view(np.uint32)
    assert added[3] == 0 and added[COUNTED].tolist() == (64 * want["stats"][COUNTED].astype(np.int64)).tolist()


def test_pick_on_257_x_130(hotpath):
    """Seeded points, the four corners, clamped out-of-range points and a duplicated point in one call; then one point; then none."""
    import torch
    w, h, seed = G.SOUPS[1]
    draws, view, proj, depth, _ = soup_reference(w, h, seed)
    want = O.image(draws, view, proj, depth, w, h)
    sel = every_slot(device_draws(draws))
    points = mixed_points(w, h, 21, want["keys"] != 0)
    got = run_pick(hotpath, sel, view, proj, depth, w, h, points)
    same_pick(got, want, points, w, h, "64 points")
    assert np.array_equal(got[0][9], got[0][63]) and (got[0][:, 1] != 0).sum() >= 28
    same_pick(run_pick(hotpath, sel, view, proj, depth, w, h, points[12:13]), want, points[12:13], w, h, "1 point")
    records, added = run_pick(hotpath, sel, view, proj, depth, w, h, [])
    assert records.shape == (0, 4) and not added.any()
    untouched = torch.full((4, 4), POISON, dtype=torch.int32, device="cuda")
    hotpath.object_id_pick(sel, view, proj, _device(depth), w, h, np.zeros((0, 2), np.int64), results=untouched)
    torch.cuda.synchronize()
    assert bool((untouched == POISON).all())


@pytest.mark.parametrize("w,h", R.TARGETS)
def test_pick_on_the_strip_through_the_near_plane(hotpath, w, h):
    """raycast_ref's strip: cut triangles (two pieces under one key) and two triangles larger than the target that cross the near plane."""
    sc, _ = R.cast_scene("near-plane strip", w, h)
    depth, _ = D.depth_prepass(sc.draws, sc.view, sc.proj, w, h)
    want = O.image(sc.draws, sc.view, sc.proj, depth, w, h)
    assert want["stats"][4] > 0 and want["stats"][5] > 0
    sel = every_slot(device_draws(sc.draws))
    same_image(run_image(hotpath, sel, sc.view, sc.proj, depth, w, h), want, f"strip {w}x{h}")
    for seed in (1, 2):
        points = mixed_points(w, h, seed, want["keys"] != 0)
        same_pick(run_pick(hotpath, sel, sc.view, sc.proj, depth, w, h, points), want, points, w, h, f"strip {w}x{h}, points {seed}")


# ---- the walk both kernels share -------------------------------------------------------------------------------------------------------------

def _walk_commands(w, h):
    """Eight commands of at most 70 triangles on a w x h target under hand_camera, one per refusal or skip of the walk over the draws, and
    two good ones: 0 a stride of 32, 1 an R16 index format, 2 an index range of 6 triangles over an index buffer of 3, 3 two triangles with
    a vertex past the vertex buffer, 4 InstanceCount 0, 5 seventy triangles (more than 1 << 6), 6 sixty-five (a second chunk), 7 sixty.
    Seeded triangles of both windings with edges up to half the target, at view depths 1, 2 and 4, some cut by the near plane or behind it."""
    rng = np.random.default_rng(16)

    def triangles(n):
        corner = rng.uniform(-2.0, w + 2.0, (n, 1, 2))
        xy = corner + rng.uniform(-0.5 * w, 0.5 * w, (n, 3, 2)) * rng.uniform(0.05, 1.0, (n, 1, 1))
        z = rng.choice([1.0, 2.0, 4.0], (n, 3))
        z[(rng.uniform(size=(n, 3)) < 0.1) | (rng.uniform(size=(n, 1)) < 0.05)] = 0.5 * D.NEAR  # behind the near plane: a vertex, or all three
        return np.array([D.at(x, y, zz, w, h) for (x, y), zz in zip(xy.reshape(-1, 2), z.reshape(-1))], np.float32)

    def draw(n, oid, **kw):
        return G.GDraw(G.vertex_buffer(triangles(n)), np.arange(3 * n, dtype=np.uint32), object_id=oid, **kw)

    short = G.GDraw(D.S.vertex_buffer(triangles(4), stride=32), np.arange(12, dtype=np.uint32), stride=32, object_id=10)
    past_vb = draw(6, 13)
    past_vb.indices[4], past_vb.indices[15] = 18, 0x7FFFFFF0  # triangles 1 and 5: one vertex behind the last, one far behind
    return [short, draw(4, 11, index_format=57), draw(3, 12, index_count=18), past_vb, draw(5, 14, instance_count=0), draw(70, 15), draw(65, 16), draw(60, 17)]


@pytest.mark.parametrize("bits,refused", [(7, 4 + 4 + 3 + 2), (6, 4 + 4 + 3 + 2 + 70 + 65)])
def test_refusals_of_the_shared_walk_from_both_kernels(hotpath, bits, refused):
    """ur_object_id_pass and ur_object_id_pick (four calls of 64 points: every texel of 16 x 16) over _walk_commands under every slot, a
    list and ranges give the restatement's records and counters. With 7 triangle bits the commands of 70 and 65 triangles are drawn, the
    latter through a second chunk; with 6 both are refused as a whole, so stats[1] is worked by hand for both."""
    from unclerenderer_amd.hotpath import raster_draws, to_device
    w = h = 16
    draws = _walk_commands(w, h)
    assert len(draws) == 8 and max(d.count() // 3 for d in draws) == 70
    view, proj = D.hand_camera(w, h)
    rng = np.random.default_rng(3)
    depth = np.where(rng.uniform(size=(h, w)) < 0.3, np.float32(D.NEAR / 1.5), np.float32(0.0)).astype(np.float32)  # (behind it: view depths 2 and 4)
    dd = device_draws(draws)
    base = 1000
    idx = np.array([base + k for k in (7, 5, 0, 6, 2, 1, 3, 4)], np.uint32)
    offsets, counts = np.array([0, 3, 3, 8], np.uint32), np.array([3, 0, 5], np.uint32)
    compacted = to_device(dd.host_commands.view(np.int32).copy())
    selections = [("every slot", None, raster_draws(dd.commands)),
                  ("list", G.selection(8, visible=(idx, 8), index_base=base), raster_draws(dd.commands, None, (to_device(idx), to_device(np.array([8], np.uint32))), None, base)),
                  ("ranges", G.selection(8, ranges=(offsets, counts)), raster_draws(None, None, None, (to_device(offsets), compacted, to_device(counts))))]
    assert [s for _, s in selections[1][1]] == [7, 5, 0, 6, 2, 1, 3, 4] and [s for _, s in selections[2][1]] == list(range(8))
    calls = O.every_texel(w, h)
    assert len(calls) == 4
    for name, select, sel in selections:
        want = O.image(draws, view, proj, depth, w, h, select=select, key_triangle_bits=bits)
        ids = set(want["object_id"].reshape(-1).tolist())
        assert want["stats"][1] == refused and want["stats"][0] > 0 and want["stats"][4] > 0 and want["stats"][5] > 0 and 17 in ids and (16 in ids) == (bits == 7) and not ids & {10, 11, 14}, (name, want["stats"].tolist(), ids)
        same_image(run_image(hotpath, sel, view, proj, depth, w, h, key_triangle_bits=bits), want, f"{name}, {bits} bits")
        total = np.zeros(6, np.int64)
        for k, points in enumerate(calls):
            got = run_pick(hotpath, sel, view, proj, depth, w, h, points, key_triangle_bits=bits)
            same_pick(got, want, points, w, h, f"{name}, {bits} bits, call {k}")
            total += got[1]
        assert total[3] == 0 and total[COUNTED].tolist() == (4 * want["stats"][COUNTED].astype(np.int64)).tolist()


# ---- held independently by the ray casters ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", R.TARGETS)
@pytest.mark.parametrize("name,order", [("icosphere", (0,)), ("torus", (0,)), ("two draws", (0, 1)), ("two draws", (1, 0)), ("near-plane strip", (0, 1))])
def test_opaque_scenes_against_the_ray_caster(hotpath, record_property, name, order, w, h):
    import torch
    sc, rc = R.cast_scene(name, w, h)
    compared, want, left_out = OR.opaque_expectation(sc, rc)
    dd = device_draws([sc.draws[k] for k in order])
    depth = torch.full((h, w), float("nan"), dtype=torch.float32, device="cuda")
    hotpath.depth_prepass(sc.view, sc.proj, dd.commands, depth)  # same stream, no synchronisation in between
    got = run_image(hotpath, every_slot(dd), sc.view, sc.proj, depth, w, h)
    record_property(f"{name} {order} {w}x{h}", f"left out {left_out:.2%}")
    assert left_out <= R.LEFT_OUT_CAP
    assert (compared & (want != 0)).any() and OR.held(got["object_id"], compared, want) == 0


@pytest.mark.parametrize("w,h", R.TARGETS)
@pytest.mark.parametrize("order_name", sorted(OR.MASKED_ORDERS))
def test_masked_scene_against_the_ray_caster(hotpath, record_property, order_name, w, h):
    """ur_depth_prepass over the opaque draw, ur_gbuffer_pass_masked raising it, ur_object_id_pass over all three draws against that."""
    import torch
    sc, rc = T.cast_scene("masked", w, h)
    moved, slot_of = OR.reordered(sc, OR.MASKED_ORDERS[order_name])
    dd = device_draws(moved.draws)
    msel = gbuffer_mask_gpu.Selections(dd, moved.opaque, list(moved.masked))
    depth = torch.full((h, w), float("nan"), dtype=torch.float32, device="cuda")
    hotpath.depth_prepass(moved.view, moved.proj, msel.call_commands, depth, **msel.opaque)
    gbuf = gbuffer_mask_gpu.run(hotpath, msel, device_materials(T.ref_materials(moved.mats)), moved.view, moved.proj, depth.cpu().numpy(), w, h)
    got = run_image(hotpath, every_slot(dd), moved.view, moved.proj, gbuf["depth"], w, h)
    compared, want, counts, ids = TO.check_masked(record_property, f"ur_object_id_pass, masked ({order_name}) {w}x{h}", sc, rc, w, h, slot_of, got["object_id"])
    if order_name == "ico, torus, grid":
        assert (want[compared] == ids["grid"]).all() and counts["grid"] == int(compared.sum()) > 0
    else:
        assert all(n > 0 for n in counts.values()), counts
        by_slot = np.array([d.object_id for d in moved.draws] + [0], np.uint32)
        gbuffer_id = by_slot[np.where(gbuf["keys"] != 0, (gbuf["keys"] >> G.key_bits(3)).astype(np.int64) - 1, 3)]
        differ = compared & (gbuf["keys"] != 0) & (got["object_id"] != gbuffer_id)
        background = compared & (gbuf["keys"] == 0) & (got["object_id"] != 0)
        record_property("differs", f"{int(differ.sum())} covered texels differ from the G-buffer's winning draw, {int(background.sum())} background texels carry an id")
        assert differ.any() and background.any()
