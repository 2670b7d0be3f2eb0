"""BC1, BC3 and BC5 maps in the material sampler on the GPU: a BC texture gives exactly the bytes of an RGBA8
texture that holds its decoded texels. ur_gbuffer_pass_materials (keys 0-15), ur_gbuffer_pass_masked and ur_forward_pass over materials of
random blocks (tests/bcn_gpu.py: the format cycles per command and per map, RGBA8 among them, so neighbouring lanes hold different
formats) are byte-equal in every output to (a) the numpy restatement over the decoded twins and (b) the same call with the twins uploaded
as RGBA8 - and differ from the run with every map bit clear, so the maps were sampled. NaN is compared by NaN-ness."""
import numpy as np
import pytest

from tests import bcn_gpu as B
from tests import bcn_ref as R
from tests import depth_ref as D
from tests import forward_ref as FW
from tests import gbuffer_mask_ref as M
from tests import gbuffer_tex_ref as X
from tests import forward_gpu, gbuffer_mask_gpu
from tests.gbuffer_gpu import device_draws, run, same

pytestmark = pytest.mark.gpu

TARGETS = ("A", "B", "C", "hdr", "keys", "object_id")
_CACHE = {}


def _depth(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to("cuda")


def _equal(got, other, what, names):
    for k in names:
        if k in got and k in other:
            a, b = np.atleast_1d(got[k]), np.atleast_1d(other[k])
            assert a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{what}: {k} differs between the BC run and the RGBA8 run"


def _materials_soup(w, h, seed):
    """(draws, view, proj, depth, BC materials, restatement over the twins), computed once and left unchanged."""
    key = ("materials", w, h, seed)
    if key not in _CACHE:
        draws = X.soup(w, h, seed)
        view, proj = D.soup_camera(w, h)
        depth, _ = D.depth_prepass(draws, view, proj, w, h)
        mats = B.bc_materials(X.soup_materials(seed, shapes=B.SHAPES), seed)
        assert B.formats_in(mats) == {28, 29, 71, 72, 77, 78, 83}
        assert {(m[n].width, m[n].height, len(m[n].levels)) for m in mats for n, _, _ in X.MAPS if m[n].data is not None} == set(B.SHAPES)
        want = X.gbuffer_pass(draws, view, proj, depth, w, h, materials=mats)
        _CACHE[key] = (draws, view, proj, depth, mats, want)
    return _CACHE[key]


@pytest.mark.parametrize("w,h,seed", X.SOUPS)
def test_gbuffer_pass_materials(hotpath, w, h, seed):
    draws, view, proj, depth, mats, want = _materials_soup(w, h, seed)
    dd, dev_depth = device_draws(draws), _depth(depth)
    bc, twins, clear = B.device_materials(mats), B.device_materials(mats, as_rgba8=True), B.device_materials([{"key": 0} for _ in mats])
    for oid in (True, False):
        got = run(hotpath, dd, view, proj, dev_depth, w, h, object_id=oid, materials=bc)
        same(got, want, f"BC soup {w}x{h}, ObjectId {oid}")
        _equal(got, run(hotpath, dd, view, proj, dev_depth, w, h, object_id=oid, materials=twins), f"soup {w}x{h}", TARGETS + ("stats",))
    plain = run(hotpath, dd, view, proj, dev_depth, w, h, materials=clear)
    assert np.array_equal(plain["keys"], got["keys"])
    for k in ("A", "B", "C", "hdr"):  # normal, metallic-roughness, base colour and emissive maps: none of them white
        assert not np.array_equal(plain[k], got[k]), f"{k}: the BC run equals the run with every map bit clear"
    if h > 78:  # bands against the whole frame (an odd row0: the quads stay anchored at even frame rows)
        for row0, rows in ((0, 37), (37, 41), (78, 52)):
            band = run(hotpath, dd, view, proj, dev_depth, w, h, row0, rows, materials=bc)
            same(band, want, f"BC soup rows [{row0}, {row0 + rows})", row0, rows)


def test_the_resolve_part_alone(hotpath):
    """ur_gbuffer_pass_materials_parts: the raster part reads no material, the resolve part alone leaves ur_gbuffer_pass_materials' bytes."""
    import torch
    from unclerenderer_amd import lib
    from unclerenderer_amd.hotpath import gbuffer_targets
    w, h, seed = X.SOUPS[0]
    draws, view, proj, depth, mats, want = _materials_soup(w, h, seed)
    dd, dm, dev_depth = device_draws(draws), B.device_materials(mats), _depth(depth)
    half = lambda: torch.full((h, w, 4), float("nan"), dtype=torch.float16, device="cuda")  # noqa: E731
    word = lambda: torch.full((h, w), 0x5A5A5A5A, dtype=torch.int32, device="cuda")  # noqa: E731
    a, b, hdr, c, keys, oid = half(), half(), half(), word(), word(), word()
    stats = torch.zeros(6, dtype=torch.int32, device="cuda")
    tg = gbuffer_targets(a, b, c, hdr, keys, oid)
    hotpath.gbuffer_pass(view, proj, dd.commands, dev_depth, tg, w, h, stats=stats, parts=lib.UR_GBUFFER_PART_RASTER, materials=dm)
    torch.cuda.synchronize()
    assert np.array_equal(keys.cpu().numpy().view(np.uint32), want["keys"]) and bool(torch.isnan(hdr).all()) and bool((c == 0x5A5A5A5A).all())
    counted = stats.cpu().numpy().copy()
    hotpath.gbuffer_pass(view, proj, dd.commands, dev_depth, tg, w, h, stats=stats, parts=lib.UR_GBUFFER_PART_RESOLVE, materials=dm)
    torch.cuda.synchronize()
    got = {"A": a, "B": b, "hdr": hdr, "C": c, "keys": keys, "object_id": oid}
    got = {k: t.cpu().numpy().view(np.uint16 if t.dtype == torch.float16 else np.uint32) for k, t in got.items()}
    got["stats"] = counted.view(np.uint32)
    assert np.array_equal(stats.cpu().numpy(), counted)
    same(got, want, "BC: raster part, then resolve part")


def _masked_soup(w, h, seed):
    key = ("masked", w, h, seed)
    if key not in _CACHE:
        draws = M.soup(w, h, seed)
        opaque, masked = M.soup_selections()
        slots = [s for _, s in masked]
        base = [dict(m) for m in X.soup_materials(seed, shapes=B.SHAPES)]
        for k in slots:  # gbuffer_mask_ref.soup_materials' keys, with a base-colour map on three more of the alpha-tested slots
            if k != 14:
                base[k]["key"] |= M.ALPHA_MASK | (X.BASE_COLOR if k in (2, 8, 11) else 0)
        mats = B.bc_materials(base, seed + 50, masked_slots=slots)
        tested = [mats[k]["base_color"] for k in slots if mats[k]["key"] & M.ALPHA_MASK and mats[k]["key"] & X.BASE_COLOR]
        assert {t.fmt for t in tested} >= {R.BC1_SRGB, R.BC3_SRGB}  # punch-through BC1 and BC3 alpha under the alpha test
        for t in tested:
            if t.fmt == R.BC1_SRGB:  # punch-through: transparent and opaque texels side by side
                alpha = np.concatenate([lv[:, :, 3].reshape(-1) for lv in t.levels])
                assert (alpha == 0).any() and (alpha == 255).any() and set(alpha.tolist()) == {0, 255}
        view, proj = D.soup_camera(w, h)
        depth, _ = D.depth_prepass(draws, view, proj, w, h, slots=[s for _, s in opaque])
        want = M.masked_pass(draws, view, proj, depth, w, h, materials=mats, select=opaque, mask_select=masked)
        _CACHE[key] = (draws, mats, opaque, masked, view, proj, depth, want)
    return _CACHE[key]


MASKED_OUTPUTS = ("A", "B", "C", "hdr", "keys", "keys64", "depth", "stats", "mask_stats", "won")


@pytest.mark.parametrize("w,h,seed", M.SOUPS)
def test_gbuffer_pass_masked(hotpath, w, h, seed):
    """The alpha test reads channel A of BC1 punch-through blocks (0 or 255) and of BC3's alpha blocks through the masked raster; COLOR.a in
    [0.25, 1.25) and BaseColorAlpha in [0.8, 1.2) put the product on both sides of the cutoffs in (0.2, 0.8)."""
    draws, mats, opaque, masked, view, proj, depth, want = _masked_soup(w, h, seed)
    dd = device_draws(draws)
    sel = gbuffer_mask_gpu.Selections(dd, [s for _, s in opaque], [s for _, s in masked])
    assert 0 < int(want["wins"].sum()) and want["mask_stats"][0] > 0
    hotpath.raster_reserve(4096)
    try:
        got = gbuffer_mask_gpu.run(hotpath, sel, B.device_materials(mats), view, proj, depth, w, h)
        gbuffer_mask_gpu.same_masked(got, want, depth, f"BC masked soup {w}x{h}")
        twin = gbuffer_mask_gpu.run(hotpath, sel, B.device_materials(mats, as_rgba8=True), view, proj, depth, w, h)
        _equal(got, twin, f"masked soup {w}x{h}", MASKED_OUTPUTS)
        assert got["won"] == twin["won"]
        opaque_alpha = gbuffer_mask_gpu.run(hotpath, sel, B.device_materials([{"key": m["key"] & M.ALPHA_MASK} for m in mats]), view, proj, depth, w, h)
        assert opaque_alpha["won"] != got["won"] and not np.array_equal(opaque_alpha["keys"], got["keys"])  # the maps' alpha discarded fragments
        if h > 78:
            for row0, rows in ((0, 37), (37, 41), (78, 52)):
                band = gbuffer_mask_gpu.run(hotpath, sel, B.device_materials(mats), view, proj, depth, w, h, row0, rows)
                gbuffer_mask_gpu.same_masked(band, want, depth, f"BC masked rows [{row0}, {row0 + rows})", row0, rows)
    finally:
        hotpath.raster_reserve(0)


@pytest.mark.parametrize("w,h,seed", FW.SOUPS)
def test_forward_pass(hotpath, w, h, seed):
    draws, mats, opaque, masked, view, proj, depth, _ = _masked_soup(w, h, seed)
    frm = FW.soup_frame(w, h, seed)
    background = np.random.default_rng(5).integers(0, 0x7800, (h, w, 4)).astype(np.uint16)
    want = FW.forward_pass(draws, view, proj, depth, w, h, frm, materials=mats, select=opaque, mask_select=masked, hdr=background)
    dd = device_draws(draws)
    sel = gbuffer_mask_gpu.Selections(dd, [s for _, s in opaque], [s for _, s in masked])
    dframe = forward_gpu.DeviceFrame(hotpath, frm)
    hotpath.raster_reserve(4096)
    try:
        got = forward_gpu.run(hotpath, sel, B.device_materials(mats), view, proj, depth, w, h, dframe, background)
        forward_gpu.same_forward(got, want, depth, f"BC forward soup {w}x{h}")
        twin = forward_gpu.run(hotpath, sel, B.device_materials(mats, as_rgba8=True), view, proj, depth, w, h, dframe, background)
        _equal(got, twin, f"forward soup {w}x{h}", ("hdr", "keys", "keys64", "depth", "stats", "mask_stats"))
        assert got["won"] == twin["won"]
        clear = forward_gpu.run(hotpath, sel, B.device_materials([{"key": m["key"] & M.ALPHA_MASK} for m in mats]), view, proj, depth, w, h, dframe, background)
        assert not np.array_equal(clear["hdr"], got["hdr"])
        if h > 78:
            band = forward_gpu.run(hotpath, sel, B.device_materials(mats), view, proj, depth, w, h, dframe, background, 37, 41)
            forward_gpu.same_forward(band, want, depth, "BC forward rows [37, 78)", 37, 41)
    finally:
        hotpath.raster_reserve(0)


RANGE_END_CASES = ["nan_u_one_level", "nan_u_four_levels", "inf_v", "nan_uv", "limit_kept_positive", "limit_dropped_positive", "limit_kept_negative",
                   "limit_dropped_negative", "huge_gradient", "huge_gradient_past_limit", "chain33_nan", "chain33_gradient_2p30", "chain255_nan",
                   "chain255_gradient_2p30", "chain40_gradient_2p33"]


def range_end_case(name, kind):
    """A hand case of tests/test_gbuffer_tex_ref.py (NaN and infinite coordinates, the 2^30 limit on both sides, chains of 33 and 255
    levels read at their far end) with its emissive map replaced by blocks of the same shape."""
    from tests.test_gbuffer_tex_ref import hand_cases
    draws, mats = hand_cases()[name]
    t = mats[0]["emissive"]
    return draws, [{"key": mats[0]["key"], "emissive": B.bc_texture(kind, t.width, t.height, len(t.levels), kind != "bc5", 900 + len(name))}]


@pytest.mark.parametrize("kind", ["bc1", "bc3", "bc5"])
def test_coordinates_and_chains_at_the_ends_of_their_ranges(hotpath, kind):
    from tests.test_gbuffer_tex_ref import H, W
    cam = D.hand_camera(W, H)
    for name in RANGE_END_CASES:
        draws, mats = range_end_case(name, kind)
        depth, _ = D.depth_prepass(draws, *cam, W, H)
        want = X.gbuffer_pass(draws, *cam, depth, W, H, materials=mats)
        dd = device_draws(draws)
        got = run(hotpath, dd, *cam, _depth(depth), W, H, materials=B.device_materials(mats))
        same(got, want, f"{name}, {kind}")
        _equal(got, run(hotpath, dd, *cam, _depth(depth), W, H, materials=B.device_materials(mats, as_rgba8=True)), f"{name}, {kind}", TARGETS)
        assert not np.array_equal(got["hdr"], run(hotpath, dd, *cam, _depth(depth), W, H, materials=B.device_materials([{"key": 0}]))["hdr"]), name


def test_the_widest_and_the_tallest_bc1_map(hotpath):
    """65535 x 1 and 1 x 65535 with 17 levels (16384 blocks in a row, in a column; level 16 is the chain's last block), on every map."""
    w, h, seed = X.SOUPS[0]
    draws, view, proj, depth, _, _ = _materials_soup(w, h, seed)
    mats = B.bc_materials(X.soup_materials(seed, shapes=[(65535, 1, 17), (1, 65535, 17)]), seed + 7, shapes=[(65535, 1, 17), (1, 65535, 17)], kinds=("bc1",))
    assert B.formats_in(mats) == {R.BC1, R.BC1_SRGB}
    want = X.gbuffer_pass(draws, view, proj, depth, w, h, materials=mats)
    dd = device_draws(draws)
    got = run(hotpath, dd, view, proj, _depth(depth), w, h, materials=B.device_materials(mats))
    same(got, want, "65535 x 1 and 1 x 65535 BC1")
    _equal(got, run(hotpath, dd, view, proj, _depth(depth), w, h, materials=B.device_materials(mats, as_rgba8=True)), "65535", TARGETS)


def test_an_address_aligned_to_half_a_block_is_a_clear_bit(hotpath):
    """BC1 at 4 but not 8 bytes, BC3 and BC5 at 8 but not 16: the descriptor is invalid and its bit counts as clear, in all three families;
    the same chains at their own alignment are sampled."""
    w, h, seed = X.SOUPS[0]
    draws, mats, opaque, masked, view, proj, depth, _ = _masked_soup(w, h, seed)
    broken, hit = [dict(m) for m in mats], set()
    for k, m in enumerate(broken):
        for name, bit, _ in X.MAPS:
            t = m.get(name)
            if t is not None and t.data is not None and m["key"] & bit and (k + bit) % 2 == 0:
                m[name] = B.BcTex(t.levels, t.srgb, valid=False, how="misaligned", fmt=t.fmt, data=t.data)
                hit.add((R.block_bytes(t.fmt), name))
    assert hit >= {(8, "base_color"), (16, "base_color"), (8, "normal"), (16, "emissive")}
    dd = device_draws(draws)
    sel = gbuffer_mask_gpu.Selections(dd, [s for _, s in opaque], [s for _, s in masked])
    dm = B.device_materials(broken)
    want = M.masked_pass(draws, view, proj, depth, w, h, materials=broken, select=opaque, mask_select=masked)
    got = gbuffer_mask_gpu.run(hotpath, sel, dm, view, proj, depth, w, h)
    gbuffer_mask_gpu.same_masked(got, want, depth, "misaligned BC descriptors, masked")
    aligned = gbuffer_mask_gpu.run(hotpath, sel, B.device_materials(mats), view, proj, depth, w, h)
    assert not np.array_equal(aligned["C"], got["C"]) and aligned["won"] != got["won"]
    frm = FW.soup_frame(w, h, seed)
    background = np.full((h, w, 4), FW.POISON_HDR, np.uint16)
    want = FW.forward_pass(draws, view, proj, depth, w, h, frm, materials=broken, select=opaque, mask_select=masked, hdr=background)
    got = forward_gpu.run(hotpath, sel, dm, view, proj, depth, w, h, forward_gpu.DeviceFrame(hotpath, frm), background)
    forward_gpu.same_forward(got, want, depth, "misaligned BC descriptors, forward")
    plain_depth, _ = D.depth_prepass(draws, view, proj, w, h)
    want = X.gbuffer_pass(draws, view, proj, plain_depth, w, h, materials=[dict(m, key=m["key"] & 15) for m in broken])
    same(run(hotpath, dd, view, proj, _depth(plain_depth), w, h, materials=dm), want, "misaligned BC descriptors, materials")


def test_one_frame_with_bc_tables_equals_the_direct_calls(hotpath):
    """Frame.set_gbuffer_materials passes the table through untouched: a frame of cull -> DepthPrepass -> GBuffer -> Lighting -> Sky with BC
    tables leaves the direct call's G-buffer and the restatement's."""
    import torch
    from tests.test_gpu_gbuffer_frame import H, W
    from tests.test_gpu_gbuffer_tex_frame import _textured_scene
    from unclerenderer_amd import lib
    from unclerenderer_amd.hotpath import Frame, gbuffer_targets
    s = _textured_scene(hotpath)
    rng = np.random.default_rng(4)
    base = [{"key": 15 - 2 * k, **{name: X.random_texture(4, 4, 1, name == "base_color", rng) for name, _, _ in X.MAPS}} for k in range(s.n)]
    mats = B.bc_materials(base, 21, shapes=[(20, 12, 5), (64, 64, 7), (3, 5, 3)], kinds=("bc1", "bc3", "bc5"))
    dm = B.device_materials(mats)
    flags = lib.UR_FRAME_DEFAULT | lib.UR_FRAME_DEPTH_PASS | lib.UR_FRAME_GBUFFER_PASS
    frame = Frame(hotpath)
    try:
        s.set_passes(frame)
        frame.set_gbuffer_materials(dm)
        s.gstats.zero_()
        s.render(frame, flags)
        depth, _ = D.depth_prepass(s.draws, s.view, s.proj, W, H)
        order = s.vis.cpu().numpy()[:int(s.cnt.cpu()[0])].tolist()
        want = X.gbuffer_pass(s.draws, s.view, s.proj, depth, W, H, materials=mats, select=list(enumerate(order)))
        got = {"A": s.a.cpu().numpy().view(np.uint16), "B": s.b.cpu().numpy().view(np.uint16), "C": s.c.cpu().numpy().view(np.uint32),
               "keys": s.keys.cpu().numpy().view(np.uint32), "object_id": s.oid.cpu().numpy().view(np.uint32), "stats": s.gstats.cpu().numpy().view(np.uint32)}
        same(got, want, "the frame's G-buffer under BC tables")
        a, b, hdr = (torch.zeros((H, W, 4), dtype=torch.float16, device="cuda") for _ in range(3))
        c, keys = (torch.zeros((H, W), dtype=torch.int32, device="cuda") for _ in range(2))
        hotpath.gbuffer_pass(s.view, s.proj, s.args, s.depth, gbuffer_targets(a, b, c, hdr, keys), W, H, visible=(s.vis, s.cnt), materials=dm)
        torch.cuda.synchronize()
        for x, y in ((a, s.a), (b, s.b), (c, s.c), (keys, s.keys)):
            assert np.array_equal(x.cpu().numpy().view(np.uint8), y.cpu().numpy().view(np.uint8))
        assert np.array_equal(hdr.cpu().numpy().view(np.uint16), want["hdr"])
    finally:
        frame.close()
