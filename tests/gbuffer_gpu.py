"""Device side of the GBuffer tests: upload tests/gbuffer_ref.py GDraws (tests/shadow_gpu.py's DeviceDraws over whole constant blocks)
and run ur_gbuffer_pass over NaN / poison filled targets."""
from __future__ import annotations

import numpy as np

from tests import gbuffer_ref as G
from tests.shadow_gpu import DeviceDraws

NAMES = ("keys", "A", "B", "C", "hdr", "object_id")


def device_draws(draws) -> DeviceDraws:
    return DeviceDraws([G.as_device_draw(d) for d in draws])


def run(hotpath, dd, view, proj, depth, w, h, row0=0, rows=None, object_id=True, **kw):
    """ur_gbuffer_pass over poisoned band targets and zeroed stats: dict like gbuffer_ref.gbuffer_pass' for the rows of the band. depth:
    a (h, w) float32 device tensor."""
    import torch
    rows = h - row0 if rows is None else rows
    half = lambda: torch.full((rows, w, 4), float("nan"), dtype=torch.float16, device="cuda")  # noqa: E731
    word = lambda: torch.full((rows, w), 0x5A5A5A5A, dtype=torch.int32, device="cuda")  # noqa: E731
    a, b, hdr, c, keys, oid = half(), half(), half(), word(), word(), (word() if object_id else None)
    stats = torch.zeros(6, dtype=torch.int32, device="cuda")
    from unclerenderer_amd.hotpath import gbuffer_targets
    tg = gbuffer_targets(a, b, c, hdr, keys, oid)
    hotpath.gbuffer_pass(view, proj, dd.commands, depth, tg, w, h, row0, rows, stats=stats, **kw)
    torch.cuda.synchronize()
    out = {"A": a.cpu().numpy().view(np.uint16), "B": b.cpu().numpy().view(np.uint16), "hdr": hdr.cpu().numpy().view(np.uint16),
           "C": c.cpu().numpy().view(np.uint32), "keys": keys.cpu().numpy().view(np.uint32), "stats": stats.cpu().numpy().view(np.uint32)}
    if oid is not None:
        out["object_id"] = oid.cpu().numpy().view(np.uint32)
    return out


def same(got, want, what, row0=0, rows=None, counted=(0, 1, 2, 4, 5)):
    """Byte equality of every output the run has (NaN compared by NaN-ness in the fp16 targets) and of the counted stats."""
    for k in NAMES:
        if k not in got:
            continue
        g, e = got[k], want[k][row0:(None if rows is None else row0 + rows)]
        if k in ("A", "B", "hdr"):
            gn, en = np.isnan(g.view(np.float16)), np.isnan(e.view(np.float16))
            bad = (gn != en) | (~gn & (g != e))
        else:
            bad = g != e
        if bad.any():
            at = np.argwhere(bad)[0]
            raise AssertionError(f"{what}: {k}: {int(bad.sum())} values differ, first at {tuple(int(v) for v in at)}: got {g[tuple(at)]:#x}, want {e[tuple(at)]:#x}")
    assert got["stats"][list(counted)].tolist() == want["stats"][list(counted)].tolist(), (what, got["stats"].tolist(), want["stats"].tolist())
