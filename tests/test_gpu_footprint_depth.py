"""Footprint rules (tests/footprint.py, run_rules unchanged) for ur_depth_prepass: the target, the stats, the command slots, the vertex,
index and constant buffers they point at and the list are touched only where include/ur_raster.h says.

The command slots hold the addresses of the guarded buffers of their run, so they are packed inside the call and guarded here by hand
with the run's poison; their guards and payload are checked when the runs are over."""
import numpy as np
import pytest

from tests import depth_ref as R
from tests import footprint as fp

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("reserve,flags", [(4096, 0), (0, R.QUANTIZE_D24)])
def test_depth_prepass_footprint(hotpath, reserve, flags):
    import torch
    from unclerenderer_amd.hotpath import pack_draw_commands
    w, h = 257, 130  # off every tile and stamp multiple; rows of 1028 bytes
    draws = [d for d in R.soup(w, h, 11, triangles=500) if d.instance_count]
    view, proj = R.soup_camera(w, h)
    base = 77
    idx = np.array([base + k for k in (3, 0, 2, 1)] + [base + 9], np.uint32)  # the last entry lies behind the count
    cnt = np.array([4], np.uint32)
    inputs = {"visible_idx": idx, "visible_count": cnt}
    for k, d in enumerate(draws):
        inputs[f"vertices{k}"] = np.ascontiguousarray(d.vertices).view(np.uint8)
        inputs[f"indices{k}"] = np.ascontiguousarray(d.indices, np.uint32)
        inputs[f"constants{k}"] = np.ascontiguousarray(d.world, np.float32)
    outputs = {"depth": np.full((h, w), np.nan, np.float32), "stats": np.array([5, 6, 7, 8, 9, 10], np.uint32)}
    held = []

    def call(b):
        spec = [dict(vertices=b[f"vertices{k}"], indices=b[f"indices{k}"], constants=b[f"constants{k}"], stride=d.stride, index_count=d.count(),
                     start_index=d.start_index, base_vertex=d.base_vertex) for k, d in enumerate(draws)]
        cmds = pack_draw_commands(spec)
        poison = getattr(b["visible_idx"], "footprint", None)
        dev = fp.guarded(cmds, "cuda", poison.fill) if poison is not None else fp.plain(cmds, "cuda")
        held.append((dev, cmds))
        hotpath.depth_prepass(view, proj, dev, b["depth"], visible=(b["visible_idx"], b["visible_count"]), index_base=base, stats=b["stats"], flags=flags)

    hotpath.raster_reserve(reserve)
    try:
        got = fp.run_rules(call, inputs, outputs, what=f"ur_depth_prepass, reserve {reserve}, flags {flags}")
    finally:
        torch.cuda.synchronize()
        hotpath.raster_reserve(0)
    for dev, cmds in held:
        if hasattr(dev, "footprint"):
            r = fp.check(dev)
            assert r.ok, f"command slots: {r}"
        assert np.array_equal(fp.host_bytes(dev), cmds.view(np.uint8).reshape(-1)), "the command slots were written"
    want, want_stats = R.depth_prepass(draws, view, proj, w, h, flags=flags, slots=[3, 0, 2, 1])
    assert np.array_equal(got["depth"].view(np.uint32), want.view(np.uint32))
    delta = got["stats"] - np.array([5, 6, 7, 8, 9, 10], np.uint32)
    assert delta[[0, 1, 2, 4, 5]].tolist() == want_stats[[0, 1, 2, 4, 5]].tolist()
