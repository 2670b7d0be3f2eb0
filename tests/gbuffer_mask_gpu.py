"""Device side of the alpha-masked GBuffer tests: selections as ur_raster_draws over one command buffer, and ur_gbuffer_pass_masked over
poisoned targets, a poisoned keys64 and a copy of the depth."""
from __future__ import annotations

import numpy as np

from tests.gbuffer_gpu import same

POISON64 = 0x5A5A5A5A5A5A5A5A


def slot_ranges(slots, count):
    """(offsets, counts) of ranges that select exactly the ascending `slots` of `count` commands, one range per slot (none: one empty range)."""
    if not slots:
        return np.array([0, count], np.uint32), np.array([0], np.uint32)
    return np.array(list(slots) + [count], np.uint32), np.ones(len(slots), np.uint32)


class Selections:
    """The opaque and the masked selection of one command buffer on the device, as the keyword arguments of HotPath.gbuffer_pass: kind
    "ranges" (one range per slot, the ordinal is the slot), "lists" (visible lists in the given order, the ordinal is the position)."""

    def __init__(self, dd, opaque, masked, kind="ranges", index_base=0):
        from unclerenderer_amd.hotpath import raster_draws, to_device
        n = dd.host_commands.shape[0]
        self.commands = dd.commands
        if kind == "ranges":
            (oo, oc), (mo, mc) = slot_ranges(opaque, n), slot_ranges(masked, n)
            self.opaque = dict(ranges=(to_device(oo), dd.commands, to_device(oc)))
            self.call_commands = None
            self.mask_draws = raster_draws(None, None, None, (to_device(mo), dd.commands, to_device(mc)), 0)
        else:
            lists = [(to_device(np.array([index_base + s for s in sel] + [index_base], np.uint32)), to_device(np.array([len(sel)], np.uint32))) for sel in (opaque, masked)]
            self.opaque = dict(visible=lists[0], index_base=index_base)
            self.call_commands = dd.commands
            self.mask_draws = raster_draws(dd.commands, None, lists[1], None, index_base)


def run(hotpath, sel, mats, view, proj, depth, w, h, row0=0, rows=None, **kw):
    """ur_gbuffer_pass_masked over the band: dict of keys, A, B, C, hdr, stats, mask_stats, won, keys64 (the band's rows) and depth (the
    whole frame, from a copy of `depth`)."""
    import torch
    from unclerenderer_amd.hotpath import gbuffer_targets
    rows = h - row0 if rows is None else rows
    half = lambda: torch.full((rows, w, 4), float("nan"), dtype=torch.float16, device="cuda")  # noqa: E731
    word = lambda: torch.full((rows, w), 0x5A5A5A5A, dtype=torch.int32, device="cuda")  # noqa: E731
    a, b, hdr, c, keys = half(), half(), half(), word(), word()
    keys64 = torch.full((rows, w), POISON64, dtype=torch.int64, device="cuda")
    dev_depth = torch.from_numpy(np.ascontiguousarray(depth, np.float32).copy()).to("cuda")
    stats, mask_stats = torch.zeros(6, dtype=torch.int32, device="cuda"), torch.zeros(6, dtype=torch.int32, device="cuda")
    won = torch.zeros(1, dtype=torch.int32, device="cuda")
    tg = gbuffer_targets(a, b, c, hdr, keys)
    for part in kw.pop("parts_sequence", (None,)):
        hotpath.gbuffer_pass(view, proj, sel.call_commands, dev_depth, tg, w, h, row0, rows, stats=stats, materials=mats, mask_draws=sel.mask_draws, keys64=keys64,
                             mask_stats=mask_stats, won=won, parts=part, **sel.opaque, **kw)
    torch.cuda.synchronize()
    u32 = lambda t: t.cpu().numpy().view(np.uint32)  # noqa: E731
    return {"A": a.cpu().numpy().view(np.uint16), "B": b.cpu().numpy().view(np.uint16), "hdr": hdr.cpu().numpy().view(np.uint16), "C": u32(c), "keys": u32(keys),
            "stats": u32(stats), "mask_stats": u32(mask_stats), "won": int(u32(won)[0]), "keys64": keys64.cpu().numpy().view(np.uint64),
            "depth": dev_depth.cpu().numpy()}


def same_masked(got, want, depth_before, what, row0=0, rows=None):
    """Byte equality with gbuffer_mask_ref.masked_pass' result over the band: the targets and opaque counters (gbuffer_gpu.same), keys64,
    won, the masked counters, the band's rows of depth, and the rows of depth outside the band left as they were."""
    h = want["keys"].shape[0]
    rows = h - row0 if rows is None else rows
    band = slice(row0, row0 + rows)
    same(got, want, what, row0, rows)
    assert np.array_equal(got["keys64"], want["keys64"][band]), f"{what}: keys64"
    assert got["won"] == int(want["wins"][band].sum()), (what, got["won"], int(want["wins"][band].sum()))
    counted = [0, 1, 2, 4, 5]
    assert got["mask_stats"][counted].tolist() == want["mask_stats"][counted].tolist(), (what, got["mask_stats"].tolist(), want["mask_stats"].tolist())
    before = np.asarray(depth_before, np.float32)
    assert np.array_equal(got["depth"][band].view(np.uint32), want["depth"][band].view(np.uint32)), f"{what}: depth inside the band"
    outside = np.ones(h, bool)
    outside[band] = False
    assert np.array_equal(got["depth"][outside].view(np.uint32), before[outside].view(np.uint32)), f"{what}: depth outside the band"
