"""Footprint rules (tests/footprint.py, run_rules unchanged) for the three entry-point families over BC textures:
ur_gbuffer_pass_materials, ur_gbuffer_pass_masked and ur_forward_pass read whole blocks inside the bytes of a chain and nothing around
them. Guards stand around every block chain and the material table, under both guard fills; the coordinates and chains at the ends of
their ranges are among the cases. What tests/test_gpu_footprint_gbuffer_tex.py, _gbuffer_mask.py and _forward.py guard is guarded here too.

The command slots and the material table hold the addresses of the guarded buffers of their run, so they are packed inside the call and
guarded here by hand with the run's poison; their guards and payload are checked when the runs are over."""
import numpy as np
import pytest

from tests import bcn_gpu as B
from tests import depth_ref as D
from tests import footprint as fp
from tests import forward_ref as FW
from tests import gbuffer_mask_ref as M
from tests import gbuffer_tex_ref as X
from tests.forward_gpu import same_half
from tests.gbuffer_mask_gpu import slot_ranges

pytestmark = pytest.mark.gpu

STATS0 = np.array([5, 6, 7, 8, 9, 10], np.uint32)
COUNTED = [0, 1, 2, 4, 5]


def _guarded_run(hotpath, family, draws, mats, view, proj, depth, w, h, band, reserve, flags, what, opaque=None, masked=None, frm=None, background=None):
    """fp.run_rules on one call of `family` ("materials", "masked" or "forward") with every buffer guarded. Returns the plain run's outputs."""
    import torch
    from unclerenderer_amd import lib
    from unclerenderer_amd.hotpath import forward_targets, gbuffer_targets, pack_draw_commands, raster_draws
    row0, rows = band
    n = len(draws)
    inputs = {}
    if family != "materials":
        (oo, oc), (mo, mc) = slot_ranges(opaque, n), slot_ranges(masked, n)
        inputs.update({"opaque_offsets": oo, "opaque_counts": oc, "masked_offsets": mo, "masked_counts": mc})
    if family == "forward":
        inputs.update({"shadow": np.ascontiguousarray(frm.shadow, np.float32), "cube": hotpath.stage_env_cube(frm.cube_bits, frm.env_base, frm.env_mips).cpu().numpy(),
                       "lut": np.ascontiguousarray(frm.lut, np.uint16)})
    for k, d in enumerate(draws):
        inputs[f"vertices{k}"] = np.ascontiguousarray(d.vertices).view(np.uint8)
        inputs[f"indices{k}"] = np.ascontiguousarray(d.indices, np.uint32)
        inputs[f"constants{k}"] = d.constants()
        for name, _, _ in X.MAPS:
            if mats[k].get(name) is not None:
                inputs[f"texture{k}_{name}"] = np.ascontiguousarray(B.texture_bytes(mats[k][name]))  # the chain's blocks, byte for byte
    half = np.full((rows, w, 4), np.nan, np.float16)
    word = np.full((rows, w), 0x5A5A5A5A, np.uint32)
    if family == "forward":
        outputs = {"hdr": np.ascontiguousarray(background[row0:row0 + rows]).view(np.float16), "keys": word}
    else:
        outputs = {"A": half, "B": half.copy(), "hdr": half.copy(), "C": word, "keys": word.copy()}
    if family == "materials":
        inputs["depth"] = depth
        outputs.update({"object_id": word.copy(), "stats": STATS0})
    else:
        outputs.update({"keys64": np.full((rows, w), 0x5A5A5A5A5A5A5A5A, np.uint64).view(np.int64), "depth": np.ascontiguousarray(depth, np.float32), "stats": STATS0,
                        "mask_stats": STATS0 + 10, "won": np.array([3], np.uint32)})
    scene = frm.scene_constants() if family == "forward" else None
    held = []

    def by_hand(host, like):
        poison = getattr(like, "footprint", None)
        dev = fp.guarded(host, "cuda", poison.fill) if poison is not None else fp.plain(host, "cuda")
        held.append((dev, host))
        return dev

    def call(b):
        spec = [dict(vertices=b[f"vertices{k}"], indices=b[f"indices{k}"], constants=b[f"constants{k}"], stride=d.stride, index_count=d.count(),
                     start_index=d.start_index, base_vertex=d.base_vertex) for k, d in enumerate(draws)]
        cmds = by_hand(pack_draw_commands(spec), b["vertices0"])
        rec = (lib.Material * len(mats))()
        for k, m in enumerate(mats):
            rec[k].pipeline_key = m["key"]
            for name, _, _ in X.MAPS:
                if m.get(name) is not None:
                    assert b[f"texture{k}_{name}"].data_ptr() % 16 == 0
                    setattr(rec[k], name, B.descriptor(m[name], b[f"texture{k}_{name}"].data_ptr()))
        table = by_hand(np.frombuffer(bytes(rec), np.uint32).copy(), b["vertices0"])
        if family == "materials":
            tg = gbuffer_targets(b["A"], b["B"], b["C"], b["hdr"], b["keys"], b["object_id"])
            hotpath.gbuffer_pass(view, proj, cmds, b["depth"], tg, w, h, row0, rows, stats=b["stats"], flags=flags, materials=(table, len(mats)))
            return
        mask_draws = raster_draws(None, None, None, (b["masked_offsets"], cmds, b["masked_counts"]), 0)
        common = dict(ranges=(b["opaque_offsets"], cmds, b["opaque_counts"]), stats=b["stats"], flags=flags, materials=(table, len(mats)), mask_draws=mask_draws,
                      keys64=b["keys64"], mask_stats=b["mask_stats"], won=b["won"])
        if family == "masked":
            hotpath.gbuffer_pass(view, proj, None, b["depth"], gbuffer_targets(b["A"], b["B"], b["C"], b["hdr"], b["keys"]), w, h, row0, rows, **common)
        else:
            tables = hotpath.make_tables(b["shadow"], b["cube"], frm.env_base, frm.env_mips, b["lut"])
            hotpath.forward_pass(view, proj, None, b["depth"], forward_targets(b["hdr"], b["keys"]), w, h, row0, rows, scene=scene, tables=tables, **common)

    def untouched(result):
        if family == "materials":
            return {}
        outside = np.ones((h, w), bool)
        outside[row0:row0 + rows] = False
        left = {"depth": outside}
        if family == "forward":
            left["hdr"] = np.repeat((result["keys"] == 0)[:, :, None], 4, axis=2)
        return left

    hotpath.raster_reserve(reserve)
    try:
        got = fp.run_rules(call, inputs, outputs, untouched=untouched, what=f"{family} over BC maps, {what}, reserve {reserve}, flags {flags}, rows {band}")
    finally:
        torch.cuda.synchronize()
        hotpath.raster_reserve(0)
    for dev, host in held:
        if hasattr(dev, "footprint"):
            r = fp.check(dev)
            assert r.ok, f"command slots / material table: {r}"
        assert np.array_equal(fp.host_bytes(dev), host.view(np.uint8).reshape(-1)), "the command slots or the material table were written"
    return got


def _same_targets(got, want, rows_, names):
    for k in names:
        if k in ("A", "B", "hdr"):
            assert not same_half(got[k].view(np.uint16), want[k][rows_]).any(), k
        else:
            assert np.array_equal(got[k].view(want[k].dtype), want[k][rows_]), k


def _soup(w, h):
    draws = M.soup(w, h, 11, triangles=500)
    opaque, masked = M.soup_selections()
    base = [dict(m) for m in X.soup_materials(11, shapes=B.SHAPES)]
    for _, k in masked:
        if k != 14:
            base[k]["key"] |= M.ALPHA_MASK | (X.BASE_COLOR if k in (2, 8, 11) else 0)
    mats = B.bc_materials(base, 11, masked_slots=[s for _, s in masked])
    assert B.formats_in(mats) == {28, 29, 71, 72, 77, 78, 83}
    return draws, mats, opaque, masked, D.soup_camera(w, h)


@pytest.mark.parametrize("reserve,flags,band", [(4096, 0, (37, 41)), (0, X.G.QUANTIZE_D24, (0, 130))])
def test_gbuffer_pass_materials_footprint(hotpath, reserve, flags, band):
    w, h = 257, 130  # off every tile and stamp multiple
    row0, rows = band
    draws, mats, _, _, (view, proj) = _soup(w, h)
    mats = [dict(m, key=m["key"] & 15) for m in mats]
    depth, _ = D.depth_prepass(draws, view, proj, w, h, flags=flags)
    got = _guarded_run(hotpath, "materials", draws, mats, view, proj, depth, w, h, band, reserve, flags, "soup")
    want = X.gbuffer_pass(draws, view, proj, depth, w, h, materials=mats, flags=flags)
    _same_targets(got, want, slice(row0, row0 + rows), ("keys", "C", "object_id", "A", "B", "hdr"))
    assert (got["stats"] - STATS0)[COUNTED].tolist() == want["stats"][COUNTED].tolist()


@pytest.mark.parametrize("family", ["masked", "forward"])
def test_masked_and_forward_footprint(hotpath, family):
    w, h, band, flags = 257, 130, (37, 41), 0
    rows_ = slice(band[0], band[0] + band[1])
    draws, mats, opaque, masked, (view, proj) = _soup(w, h)
    opaque, masked = opaque[:8], masked[:4]  # a part of the draws: some texels stay uncovered
    depth, _ = D.depth_prepass(draws, view, proj, w, h, flags=flags, slots=[s for _, s in opaque])
    slots = ([s for _, s in opaque], [s for _, s in masked])
    if family == "masked":
        got = _guarded_run(hotpath, family, draws, mats, view, proj, depth, w, h, band, 4096, flags, "soup", *slots)
        want = M.masked_pass(draws, view, proj, depth, w, h, materials=mats, flags=flags, select=opaque, mask_select=masked)
        _same_targets(got, want, rows_, ("keys", "C", "A", "B", "hdr"))
    else:
        frm = FW.soup_frame(w, h, 11)
        background = np.random.default_rng(3).integers(0, 0x7800, (h, w, 4)).astype(np.uint16)
        got = _guarded_run(hotpath, family, draws, mats, view, proj, depth, w, h, band, 4096, flags, "soup", *slots, frm=frm, background=background)
        want = FW.forward_pass(draws, view, proj, depth, w, h, frm, materials=mats, flags=flags, select=opaque, mask_select=masked, hdr=background)
        _same_targets(got, want, rows_, ("keys", "hdr"))
    assert want["wins"][rows_].any()
    assert np.array_equal(got["keys64"].view(np.uint64), want["keys64"][rows_])
    assert np.array_equal(got["depth"][rows_].view(np.uint32), want["depth"][rows_].view(np.uint32))
    assert int(got["won"][0]) - 3 == int(want["wins"][rows_].sum())
    assert (got["stats"] - STATS0)[COUNTED].tolist() == want["stats"][COUNTED].tolist()
    assert (got["mask_stats"] - STATS0 - 10)[COUNTED].tolist() == want["mask_stats"][COUNTED].tolist()


def test_coordinates_and_chains_at_the_ends_of_their_ranges_stay_inside_the_chain(hotpath):
    """The hand cases whose coordinate is not finite or lies at the 2^30 limit, and the 33- and 255-level chains, over BC1, BC3 and BC5
    blocks (the kind cycles through the cases), and the widest and the tallest BC1 map: the gather stays inside the chain's bytes."""
    from tests.test_gbuffer_tex_ref import H, W
    from tests.test_gpu_gbuffer_bc import RANGE_END_CASES, range_end_case
    cam = D.hand_camera(W, H)
    for k, name in enumerate(RANGE_END_CASES):
        draws, mats = range_end_case(name, ("bc1", "bc3", "bc5")[k % 3])
        depth, _ = D.depth_prepass(draws, *cam, W, H)
        got = _guarded_run(hotpath, "materials", draws, mats, *cam, depth, W, H, (0, H), 0, 0, name)
        want = X.gbuffer_pass(draws, *cam, depth, W, H, materials=mats)
        _same_targets(got, want, slice(0, H), ("keys", "C", "object_id", "hdr"))
    w, h = X.SOUPS[0][:2]
    draws = X.soup(w, h, 11, triangles=300)
    view, proj = D.soup_camera(w, h)
    shapes = [(65535, 1, 17), (1, 65535, 17)]
    mats = B.bc_materials(X.soup_materials(11, shapes=shapes), 12, shapes=shapes, kinds=("bc1",))
    depth, _ = D.depth_prepass(draws, view, proj, w, h)
    got = _guarded_run(hotpath, "materials", draws, mats, view, proj, depth, w, h, (0, h), 0, 0, "65535 x 1 and 1 x 65535")
    want = X.gbuffer_pass(draws, view, proj, depth, w, h, materials=mats)
    _same_targets(got, want, slice(0, h), ("keys", "C", "object_id", "A", "B", "hdr"))
