"""Footprint rules (tests/footprint.py, run_rules unchanged) for ur_forward_pass: guards round hdr, keys, keys64, depth, both stats6 and won,
both selections' ranges, the material table, the command slots, the buffers they point at, every texture chain, the shadow map, the staged
cube and the LUT. keys, keys64 and the counters are written inside and nowhere else; hdr only where a key won (the uncovered texels count as
left alone); depth in the band's rows only; everything else is read inside and never written.

The command slots and the material table hold the addresses of the guarded buffers of their run, so they are packed inside the call and
guarded here by hand with the run's poison; their guards and payload are checked when the runs are over."""
import numpy as np
import pytest

from tests import depth_ref as D
from tests import footprint as fp
from tests import forward_ref as FW
from tests import gbuffer_mask_ref as M
from tests import gbuffer_tex_ref as X
from tests.forward_gpu import same_half
from tests.gbuffer_mask_gpu import slot_ranges

pytestmark = pytest.mark.gpu

STATS0 = np.array([5, 6, 7, 8, 9, 10], np.uint32)


def _guarded_run(hotpath, draws, mats, opaque, masked, view, proj, depth, frm, background, w, h, band, reserve, flags, what):
    import torch
    from unclerenderer_amd import lib
    from unclerenderer_amd.hotpath import forward_targets, pack_draw_commands, raster_draws
    row0, rows = band
    n = len(draws)
    (oo, oc), (mo, mc) = slot_ranges(opaque, n), slot_ranges(masked, n)
    staged = hotpath.stage_env_cube(frm.cube_bits, frm.env_base, frm.env_mips).cpu().numpy()
    inputs = {"opaque_offsets": oo, "opaque_counts": oc, "masked_offsets": mo, "masked_counts": mc, "shadow": np.ascontiguousarray(frm.shadow, np.float32),
              "cube": staged, "lut": np.ascontiguousarray(frm.lut, np.uint16)}
    for k, d in enumerate(draws):
        inputs[f"vertices{k}"] = np.ascontiguousarray(d.vertices).view(np.uint8)
        inputs[f"indices{k}"] = np.ascontiguousarray(d.indices, np.uint32)
        inputs[f"constants{k}"] = d.constants()
        for name, _, _ in X.MAPS:
            if mats[k].get(name) is not None:
                inputs[f"texture{k}_{name}"] = np.concatenate([a.reshape(-1) for a in mats[k][name].levels]).view(np.uint32)
    outputs = {"hdr": np.ascontiguousarray(background[row0:row0 + rows]).view(np.float16), "keys": np.full((rows, w), 0x5A5A5A5A, np.uint32),
               "keys64": np.full((rows, w), 0x5A5A5A5A5A5A5A5A, np.uint64).view(np.int64), "depth": np.ascontiguousarray(depth, np.float32), "stats": STATS0,
               "mask_stats": STATS0 + 10, "won": np.array([3], np.uint32)}
    scene = frm.scene_constants()
    held = []

    def by_hand(host, like):
        poison = getattr(like, "footprint", None)
        dev = fp.guarded(host, "cuda", poison.fill) if poison is not None else fp.plain(host, "cuda")
        held.append((dev, host))
        return dev

    def call(b):
        spec = [dict(vertices=b[f"vertices{k}"], indices=b[f"indices{k}"], constants=b[f"constants{k}"], stride=d.stride, index_count=d.count(),
                     start_index=d.start_index, base_vertex=d.base_vertex) for k, d in enumerate(draws)]
        cmds = by_hand(pack_draw_commands(spec), b["opaque_offsets"])
        rec = (lib.Material * len(mats))()
        for k, m in enumerate(mats):
            rec[k].pipeline_key = m["key"]
            for name, _, _ in X.MAPS:
                t = m.get(name)
                if t is None:
                    continue
                setattr(rec[k], name, lib.Texture2D(b[f"texture{k}_{name}"].data_ptr(), t.width, t.height, len(t.levels),
                                                    lib.UR_TEXTURE_R8G8B8A8_UNORM_SRGB if t.srgb else lib.UR_TEXTURE_R8G8B8A8_UNORM, 0))
        table = by_hand(np.frombuffer(bytes(rec), np.uint32).copy(), b["opaque_offsets"])
        tables = hotpath.make_tables(b["shadow"], b["cube"], frm.env_base, frm.env_mips, b["lut"])
        mask_draws = raster_draws(None, None, None, (b["masked_offsets"], cmds, b["masked_counts"]), 0)
        hotpath.forward_pass(view, proj, None, b["depth"], forward_targets(b["hdr"], b["keys"]), w, h, row0, rows, scene=scene, tables=tables,
                             ranges=(b["opaque_offsets"], cmds, b["opaque_counts"]), stats=b["stats"], flags=flags, materials=(table, len(mats)), mask_draws=mask_draws,
                             keys64=b["keys64"], mask_stats=b["mask_stats"], won=b["won"])

    def untouched(result):
        outside = np.ones((h, w), bool)
        outside[row0:row0 + rows] = False
        return {"depth": outside, "hdr": np.repeat((result["keys"] == 0)[:, :, None], 4, axis=2)}

    hotpath.raster_reserve(reserve)
    try:
        got = fp.run_rules(call, inputs, outputs, untouched=untouched, what=f"ur_forward_pass, {what}, reserve {reserve}, flags {flags}, rows {band}")
    finally:
        torch.cuda.synchronize()
        hotpath.raster_reserve(0)
    for dev, host in held:
        if hasattr(dev, "footprint"):
            r = fp.check(dev)
            assert r.ok, f"command slots / material table: {r}"
        assert np.array_equal(fp.host_bytes(dev), host.view(np.uint8).reshape(-1)), "the command slots or the material table were written"
    return got


@pytest.mark.parametrize("reserve,flags,band", [(4096, 0, (37, 41)), (0, X.G.QUANTIZE_D24, (0, 130))])
def test_forward_pass_footprint(hotpath, reserve, flags, band):
    w, h = 257, 130  # off every tile and stamp multiple
    row0, rows = band
    draws, mats = M.soup(w, h, 11, triangles=500), M.soup_materials(11)
    opaque, masked = M.soup_selections()
    opaque, masked = opaque[:8], masked[:4]  # a part of the draws: some texels stay uncovered
    view, proj = D.soup_camera(w, h)
    frm = FW.soup_frame(w, h, 11)
    background = np.random.default_rng(3).integers(0, 0x7800, (h, w, 4)).astype(np.uint16)
    depth, _ = D.depth_prepass(draws, view, proj, w, h, flags=flags, slots=[s for _, s in opaque])
    got = _guarded_run(hotpath, draws, mats, [s for _, s in opaque], [s for _, s in masked], view, proj, depth, frm, background, w, h, band, reserve, flags, "soup")
    want = FW.forward_pass(draws, view, proj, depth, w, h, frm, materials=mats, flags=flags, select=opaque, mask_select=masked, hdr=background)
    rows_ = slice(row0, row0 + rows)
    covered = want["keys"][rows_] != 0
    assert want["wins"][rows_].any() and 0 < covered.sum() < covered.size
    assert np.array_equal(got["keys"], want["keys"][rows_]) and np.array_equal(got["keys64"].view(np.uint64), want["keys64"][rows_])
    assert not same_half(got["hdr"].view(np.uint16), want["hdr"][rows_]).any()
    assert np.array_equal(got["depth"][rows_].view(np.uint32), want["depth"][rows_].view(np.uint32))
    assert int(got["won"][0]) - 3 == int(want["wins"][rows_].sum())
    counted = [0, 1, 2, 4, 5]
    assert (got["stats"] - STATS0)[counted].tolist() == want["stats"][counted].tolist()
    assert (got["mask_stats"] - STATS0 - 10)[counted].tolist() == want["mask_stats"][counted].tolist()
