"""Device side of the DepthPrepass tests: run ur_depth_prepass over tests/shadow_gpu.py's uploaded Draws."""
from __future__ import annotations

import numpy as np

from tests.shadow_gpu import DeviceDraws  # noqa: F401


def run(hotpath, dd, view, proj, w, h, offset_floats: int = 0, **kw):
    """ur_depth_prepass over a NaN-filled target and zeroed stats: (target (h, w) float32, stats uint32[6]). offset_floats: the target
    starts that many floats into a 16-byte aligned allocation."""
    import torch
    buf = torch.full((w * h + offset_floats + 8,), float("nan"), dtype=torch.float32, device="cuda")
    m = buf[offset_floats:offset_floats + w * h]
    stats = torch.zeros(6, dtype=torch.int32, device="cuda")
    hotpath.depth_prepass(view, proj, dd.commands, m, stats=stats, size=(w, h), **kw)
    torch.cuda.synchronize()
    whole = buf.cpu().numpy()
    assert np.isnan(whole[:offset_floats]).all() and np.isnan(whole[offset_floats + w * h:]).all(), "written outside the target"
    return whole[offset_floats:offset_floats + w * h].reshape(h, w), stats.cpu().numpy().view(np.uint32)
