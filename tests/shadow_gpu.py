"""Device side of the ShadowMap tests: upload tests/shadow_ref.py Draws, pack their command slots, run ur_shadow_map."""
from __future__ import annotations

import numpy as np


class DeviceDraws:
    """The Draws' buffers on the device (kept alive here) and their packed FIndirectDrawCommand slots."""

    def __init__(self, draws, device="cuda"):
        import torch
        from unclerenderer_amd.hotpath import pack_draw_commands
        self.draws = draws
        self.buffers = []
        spec = []
        for d in draws:
            v = torch.from_numpy(np.ascontiguousarray(d.vertices).reshape(-1).view(np.uint8).copy()).to(device)
            i = torch.from_numpy(np.ascontiguousarray(d.indices, np.uint32).view(np.int32).copy()).to(device)
            c = torch.from_numpy(np.ascontiguousarray(d.world, np.float32).reshape(-1).copy()).to(device)
            if v.numel() == 0:
                v = torch.zeros(4, dtype=torch.uint8, device=device)
            self.buffers.append((v, i, c))
            spec.append(dict(vertices=v, indices=i, constants=c, stride=d.stride, index_count=d.count(), instance_count=d.instance_count,
                             start_index=d.start_index, base_vertex=d.base_vertex, index_format=d.index_format,
                             vertex_bytes=np.ascontiguousarray(d.vertices).nbytes, index_bytes=np.asarray(d.indices).size * 4))
        self.host_commands = pack_draw_commands(spec)
        self.commands = torch.from_numpy(self.host_commands.view(np.int32).copy()).to(device)


def run(hotpath, dd: DeviceDraws, lvp, w, h, **kw):
    """ur_shadow_map over a NaN-filled map and zeroed stats: (map (h, w) float32, stats uint32[4])."""
    import torch
    m = torch.full((h, w), float("nan"), dtype=torch.float32, device="cuda")
    stats = torch.zeros(4, dtype=torch.int32, device="cuda")
    hotpath.shadow_map(lvp, dd.commands, m, stats=stats, **kw)
    torch.cuda.synchronize()
    return m.cpu().numpy(), stats.cpu().numpy().view(np.uint32)
