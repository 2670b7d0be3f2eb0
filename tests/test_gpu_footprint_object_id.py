"""Footprint rules (tests/footprint.py, run_rules unchanged) for ur_object_id_pass and ur_object_id_pick: object_id, keys, the pick's
records, the stats, depth, the command slots, the vertex, index and constant buffers they point at and the list are touched only where
include/ur_raster.h says.

The command slots hold the addresses of the guarded buffers of their run, so they are packed inside the call and guarded here by hand
with the run's poison; their guards and payload are checked when the runs are over."""
import numpy as np
import pytest

from tests import depth_ref as D
from tests import footprint as fp
from tests import gbuffer_ref as G
from tests import object_id_ref as O

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("reserve,flags,band", [(4096, 0, (37, 41)), (0, G.QUANTIZE_D24, (0, 130))])
def test_object_id_pass_and_pick_footprint(hotpath, reserve, flags, band):
    import torch
    from unclerenderer_amd.hotpath import pack_draw_commands, raster_draws
    w, h = 257, 130  # off every tile and stamp multiple
    row0, rows = band
    draws = [d for d in G.soup(w, h, 11, triangles=500) if d.instance_count and d.stride == 64]
    view, proj = D.soup_camera(w, h)
    base = 77
    order = [2, 0, 1]
    idx = np.array([base + k for k in order] + [base + 9], np.uint32)  # the last entry lies behind the count
    cnt = np.array([3], np.uint32)
    depth, _ = D.depth_prepass(draws, view, proj, w, h, flags=flags, slots=order)
    rng = np.random.default_rng(5)
    points = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w, h), (0xFFFFFFFF, 3)] + [(int(rng.integers(w)), int(rng.integers(h))) for _ in range(58)]
    inputs = {"visible_idx": idx, "visible_count": cnt, "depth": depth}
    for k, d in enumerate(draws):
        inputs[f"vertices{k}"] = np.ascontiguousarray(d.vertices).view(np.uint8)
        inputs[f"indices{k}"] = np.ascontiguousarray(d.indices, np.uint32)
        inputs[f"constants{k}"] = d.constants()
    word = np.full((rows, w), 0x5A5A5A5A, np.uint32)
    start = np.array([5, 6, 7, 8, 9, 10], np.uint32)
    outputs = {"object_id": word, "keys": word.copy(), "stats": start, "results": np.full((len(points), 4), 0x5A5A5A5A, np.uint32), "pick_stats": start.copy()}
    held = []

    def call(b):
        spec = [dict(vertices=b[f"vertices{k}"], indices=b[f"indices{k}"], constants=b[f"constants{k}"], stride=d.stride, index_count=d.count(),
                     start_index=d.start_index, base_vertex=d.base_vertex) for k, d in enumerate(draws)]
        cmds = pack_draw_commands(spec)
        poison = getattr(b["visible_idx"], "footprint", None)
        dev = fp.guarded(cmds, "cuda", poison.fill) if poison is not None else fp.plain(cmds, "cuda")
        held.append((dev, cmds))
        dd = raster_draws(dev, None, (b["visible_idx"], b["visible_count"]), None, base)
        hotpath.object_id_pass(dd, view, proj, b["depth"], w, h, object_id=b["object_id"].view(torch.int32), keys=b["keys"].view(torch.int32), row0=row0, rows=rows,
                               flags=flags, stats=b["stats"])
        hotpath.object_id_pick(dd, view, proj, b["depth"], w, h, points, results=b["results"].view(torch.int32), flags=flags, stats=b["pick_stats"])

    hotpath.raster_reserve(reserve)
    try:
        got = fp.run_rules(call, inputs, outputs, what=f"ur_object_id_pass and ur_object_id_pick, reserve {reserve}, flags {flags}, rows {band}")
    finally:
        torch.cuda.synchronize()
        hotpath.raster_reserve(0)
    for dev, cmds in held:
        if hasattr(dev, "footprint"):
            r = fp.check(dev)
            assert r.ok, f"command slots: {r}"
        assert np.array_equal(fp.host_bytes(dev), cmds.view(np.uint8).reshape(-1)), "the command slots were written"
    want = O.image(draws, view, proj, depth, w, h, flags=flags, select=[(k, s) for k, s in enumerate(order)])
    for k in ("keys", "object_id"):
        assert np.array_equal(got[k], want[k][row0:row0 + rows]), k
    assert np.array_equal(got["results"], O.pick(want, points, w, h))
    counted = [0, 1, 2, 4, 5]
    assert (got["stats"] - start)[counted].tolist() == want["stats"][counted].tolist()
    assert (got["pick_stats"] - start)[counted].tolist() == want["stats"][counted].tolist() and got["pick_stats"][3] == start[3]
