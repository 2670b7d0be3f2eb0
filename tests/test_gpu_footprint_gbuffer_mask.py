"""Footprint rules (tests/footprint.py, run_rules unchanged) for ur_gbuffer_pass_masked: guards round keys64, depth, the band targets,
the key scratch, both stats6 and won, both selections' ranges, the material table, the command slots, the buffers they point at and every
texture chain. keys64, the targets, keys and the counters are written inside and nowhere else; depth is written in the band's rows only
(the rows outside count as left alone) and nothing round it; everything else is read inside and never written.

The command slots and the material table hold the addresses of the guarded buffers of their run, so they are packed inside the call and
guarded here by hand with the run's poison; their guards and payload are checked when the runs are over."""
import numpy as np
import pytest

from tests import depth_ref as D
from tests import footprint as fp
from tests import gbuffer_mask_ref as M
from tests import gbuffer_tex_ref as X
from tests.gbuffer_mask_gpu import slot_ranges

pytestmark = pytest.mark.gpu

STATS0 = np.array([5, 6, 7, 8, 9, 10], np.uint32)


def _guarded_run(hotpath, draws, mats, opaque, masked, view, proj, depth, w, h, band, reserve, flags, what):
    import torch
    from unclerenderer_amd import lib
    from unclerenderer_amd.hotpath import gbuffer_targets, pack_draw_commands, raster_draws
    row0, rows = band
    n = len(draws)
    (oo, oc), (mo, mc) = slot_ranges(opaque, n), slot_ranges(masked, n)
    inputs = {"opaque_offsets": oo, "opaque_counts": oc, "masked_offsets": mo, "masked_counts": mc}
    for k, d in enumerate(draws):
        inputs[f"vertices{k}"] = np.ascontiguousarray(d.vertices).view(np.uint8)
        inputs[f"indices{k}"] = np.ascontiguousarray(d.indices, np.uint32)
        inputs[f"constants{k}"] = d.constants()
        for name, _, _ in X.MAPS:
            if mats[k].get(name) is not None:
                inputs[f"texture{k}_{name}"] = np.concatenate([a.reshape(-1) for a in mats[k][name].levels]).view(np.uint32)
    half = np.full((rows, w, 4), np.nan, np.float16)
    word = np.full((rows, w), 0x5A5A5A5A, np.uint32)
    outputs = {"A": half, "B": half.copy(), "hdr": half.copy(), "C": word, "keys": word.copy(), "keys64": np.full((rows, w), 0x5A5A5A5A5A5A5A5A, np.uint64).view(np.int64),
               "depth": np.ascontiguousarray(depth, np.float32), "stats": STATS0, "mask_stats": STATS0 + 10, "won": np.array([3], np.uint32)}
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
        tg = gbuffer_targets(b["A"], b["B"], b["C"], b["hdr"], b["keys"])
        mask_draws = raster_draws(None, None, None, (b["masked_offsets"], cmds, b["masked_counts"]), 0)
        hotpath.gbuffer_pass(view, proj, None, b["depth"], tg, w, h, row0, rows, ranges=(b["opaque_offsets"], cmds, b["opaque_counts"]), stats=b["stats"], flags=flags,
                             materials=(table, len(mats)), mask_draws=mask_draws, keys64=b["keys64"], mask_stats=b["mask_stats"], won=b["won"])

    def untouched(result):
        outside = np.ones((h, w), bool)
        outside[row0:row0 + rows] = False
        return {"depth": outside}

    hotpath.raster_reserve(reserve)
    try:
        got = fp.run_rules(call, inputs, outputs, untouched=untouched, what=f"ur_gbuffer_pass_masked, {what}, reserve {reserve}, flags {flags}, rows {band}")
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
def test_gbuffer_pass_masked_footprint(hotpath, reserve, flags, band):
    w, h = 257, 130  # off every tile and stamp multiple
    row0, rows = band
    draws, mats = M.soup(w, h, 11, triangles=500), M.soup_materials(11)
    opaque, masked = M.soup_selections()
    view, proj = D.soup_camera(w, h)
    depth, _ = D.depth_prepass(draws, view, proj, w, h, flags=flags, slots=[s for _, s in opaque])
    got = _guarded_run(hotpath, draws, mats, [s for _, s in opaque], [s for _, s in masked], view, proj, depth, w, h, band, reserve, flags, "soup")
    want = M.masked_pass(draws, view, proj, depth, w, h, materials=mats, flags=flags, select=opaque, mask_select=masked)
    rows_ = slice(row0, row0 + rows)
    assert any(layer["sampled"].any() for layer in want["layers"]) and want["wins"][rows_].any()
    for k in ("keys", "C"):
        assert np.array_equal(got[k], want[k][rows_]), k
    assert np.array_equal(got["keys64"].view(np.uint64), want["keys64"][rows_])
    assert np.array_equal(got["depth"][rows_].view(np.uint32), want["depth"][rows_].view(np.uint32))
    assert int(got["won"][0]) - 3 == int(want["wins"][rows_].sum())
    counted = [0, 1, 2, 4, 5]
    assert (got["stats"] - STATS0)[counted].tolist() == want["stats"][counted].tolist()
    assert (got["mask_stats"] - STATS0 - 10)[counted].tolist() == want["mask_stats"][counted].tolist()
