"""Footprint rules (tests/footprint.py, run_rules unchanged) for ur_gbuffer_pass: the band targets, the key scratch, the stats, depth,
the command slots, the vertex, index and constant buffers they point at and the list are touched only where include/ur_raster.h says.

The command slots hold the addresses of the guarded buffers of their run, so they are packed inside the call and guarded here by hand
with the run's poison; their guards and payload are checked when the runs are over."""
import numpy as np
import pytest

from tests import depth_ref as D
from tests import footprint as fp
from tests import gbuffer_ref as G

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("reserve,flags,band", [(4096, 0, (37, 41)), (0, G.QUANTIZE_D24, (0, 130))])
def test_gbuffer_pass_footprint(hotpath, reserve, flags, band):
    import torch
    from unclerenderer_amd.hotpath import gbuffer_targets, pack_draw_commands
    w, h = 257, 130  # off every tile and stamp multiple
    row0, rows = band
    draws = [d for d in G.soup(w, h, 11, triangles=500) if d.instance_count and d.stride == 64]
    view, proj = D.soup_camera(w, h)
    base = 77
    order = [2, 0, 1]
    idx = np.array([base + k for k in order] + [base + 9], np.uint32)  # the last entry lies behind the count
    cnt = np.array([3], np.uint32)
    depth, _ = D.depth_prepass(draws, view, proj, w, h, flags=flags, slots=order)
    inputs = {"visible_idx": idx, "visible_count": cnt, "depth": depth}
    for k, d in enumerate(draws):
        inputs[f"vertices{k}"] = np.ascontiguousarray(d.vertices).view(np.uint8)
        inputs[f"indices{k}"] = np.ascontiguousarray(d.indices, np.uint32)
        inputs[f"constants{k}"] = d.constants()
    half = np.full((rows, w, 4), np.nan, np.float16)
    word = np.full((rows, w), 0x5A5A5A5A, np.uint32)
    outputs = {"A": half, "B": half.copy(), "hdr": half.copy(), "C": word, "keys": word.copy(), "object_id": word.copy(),
               "stats": np.array([5, 6, 7, 8, 9, 10], np.uint32)}
    held = []

    def call(b):
        spec = [dict(vertices=b[f"vertices{k}"], indices=b[f"indices{k}"], constants=b[f"constants{k}"], stride=d.stride, index_count=d.count(),
                     start_index=d.start_index, base_vertex=d.base_vertex) for k, d in enumerate(draws)]
        cmds = pack_draw_commands(spec)
        poison = getattr(b["visible_idx"], "footprint", None)
        dev = fp.guarded(cmds, "cuda", poison.fill) if poison is not None else fp.plain(cmds, "cuda")
        held.append((dev, cmds))
        tg = gbuffer_targets(b["A"], b["B"], b["C"], b["hdr"], b["keys"], b["object_id"])
        hotpath.gbuffer_pass(view, proj, dev, b["depth"], tg, w, h, row0, rows, visible=(b["visible_idx"], b["visible_count"]), index_base=base,
                             stats=b["stats"], flags=flags)

    hotpath.raster_reserve(reserve)
    try:
        got = fp.run_rules(call, inputs, outputs, what=f"ur_gbuffer_pass, reserve {reserve}, flags {flags}, rows {band}")
    finally:
        torch.cuda.synchronize()
        hotpath.raster_reserve(0)
    for dev, cmds in held:
        if hasattr(dev, "footprint"):
            r = fp.check(dev)
            assert r.ok, f"command slots: {r}"
        assert np.array_equal(fp.host_bytes(dev), cmds.view(np.uint8).reshape(-1)), "the command slots were written"
    want = G.gbuffer_pass(draws, view, proj, depth, w, h, flags=flags, select=[(k, s) for k, s in enumerate(order)])
    for k in ("keys", "C", "object_id"):
        assert np.array_equal(got[k], want[k][row0:row0 + rows]), k
    for k in ("A", "B", "hdr"):
        g, e = got[k].view(np.uint16), want[k][row0:row0 + rows]
        nan = np.isnan(got[k])
        assert np.array_equal(nan, np.isnan(e.view(np.float16))) and np.array_equal(g[~nan], e[~nan]), k
    delta = got["stats"] - np.array([5, 6, 7, 8, 9, 10], np.uint32)
    assert delta[[0, 1, 2, 4, 5]].tolist() == want["stats"][[0, 1, 2, 4, 5]].tolist()
