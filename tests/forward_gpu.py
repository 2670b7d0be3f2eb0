"""Device side of the Forward tests: a forward_ref.Frame's tables on the device, and ur_forward_pass over a given HDR image, poisoned
keys and keys64 and a copy of the depth."""
from __future__ import annotations

import numpy as np

from tests.gbuffer_mask_gpu import POISON64

COUNTED = [0, 1, 2, 4, 5]  # stats6 without the structural [3]


class DeviceFrame:
    """The frame's shadow map, staged cube and LUT on the device (kept alive here), its ur_lighting_tables and ur_scene_constants."""

    def __init__(self, hotpath, frame):
        from unclerenderer_amd.hotpath import to_device
        self.shadow = to_device(np.ascontiguousarray(frame.shadow, np.float32)) if frame.shadow is not None else None
        self.cube = hotpath.stage_env_cube(frame.cube_bits, frame.env_base, frame.env_mips)
        self.lut = to_device(np.ascontiguousarray(frame.lut, np.uint16))
        self.tables = hotpath.make_tables(self.shadow, self.cube, frame.env_base, frame.env_mips, self.lut)
        self.scene = frame.scene_constants()


def run(hotpath, sel, mats, view, proj, depth, w, h, dframe, hdr_before, row0=0, rows=None, masked=True, parts_sequence=(None,), **kw):
    """ur_forward_pass over the band: dict of hdr, keys, stats, and with `masked` mask_stats, won, keys64 (the band's rows), and depth (the
    whole frame, from a copy of `depth`). hdr_before: the whole frame's (h, w, 4) uint16 image in front of the pass."""
    import torch
    from unclerenderer_amd.hotpath import forward_targets
    rows = h - row0 if rows is None else rows
    hdr = torch.from_numpy(np.ascontiguousarray(hdr_before[row0:row0 + rows], np.uint16).view(np.int16).copy()).to("cuda").view(torch.float16)
    keys = torch.full((rows, w), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    keys64 = torch.full((rows, w), POISON64, dtype=torch.int64, device="cuda")
    dev_depth = torch.from_numpy(np.ascontiguousarray(depth, np.float32).copy()).to("cuda")
    stats, mask_stats = torch.zeros(6, dtype=torch.int32, device="cuda"), torch.zeros(6, dtype=torch.int32, device="cuda")
    won = torch.zeros(1, dtype=torch.int32, device="cuda")
    tg = forward_targets(hdr, keys)
    mask = dict(mask_draws=sel.mask_draws, keys64=keys64, mask_stats=mask_stats, won=won) if masked else {}
    for part in parts_sequence:
        hotpath.forward_pass(view, proj, sel.call_commands, dev_depth, tg, w, h, row0, rows, scene=dframe.scene, tables=dframe.tables, stats=stats, materials=mats,
                             parts=part, **mask, **sel.opaque, **kw)
    torch.cuda.synchronize()
    u32 = lambda t: t.cpu().numpy().view(np.uint32)  # noqa: E731
    return {"hdr": hdr.cpu().numpy().view(np.uint16), "keys": u32(keys), "stats": u32(stats), "mask_stats": u32(mask_stats), "won": int(u32(won)[0]),
            "keys64": keys64.cpu().numpy().view(np.uint64), "depth": dev_depth.cpu().numpy()}


def same_half(got, want):
    """The positions where two RGBA16F images differ, NaN compared by NaN-ness."""
    gn, en = np.isnan(got.view(np.float16)), np.isnan(want.view(np.float16))
    return (gn != en) | (~gn & (got != want))


def same_forward(got, want, depth_before, what, row0=0, rows=None, masked=True):
    """Byte equality with forward_ref.forward_pass' result over the band: hdr (covered texels shaded, the others as they were), keys, the
    opaque counters, and with a mask keys64, won, the masked counters and depth (the rows outside the band as they were); without one,
    depth as it was."""
    h = want["keys"].shape[0]
    rows = h - row0 if rows is None else rows
    band = slice(row0, row0 + rows)
    assert np.array_equal(got["keys"], want["keys"][band]), f"{what}: keys"
    bad = same_half(got["hdr"], want["hdr"][band])
    if bad.any():
        at = np.argwhere(bad)[0]
        raise AssertionError(f"{what}: hdr: {int(bad.sum())} values differ, first at {tuple(int(v) for v in at)}: got {got['hdr'][tuple(at)]:#x}, "
                             f"want {want['hdr'][band][tuple(at)]:#x}")
    uncovered = want["keys"][band] == 0
    assert np.array_equal(got["hdr"][uncovered], want["hdr"][band][uncovered]), f"{what}: a texel no key covers changed"
    assert got["stats"][COUNTED].tolist() == want["stats"][COUNTED].tolist(), (what, got["stats"].tolist(), want["stats"].tolist())
    before = np.asarray(depth_before, np.float32)
    if not masked:
        assert np.array_equal(got["depth"].view(np.uint32), before.view(np.uint32)), f"{what}: depth was written without a mask"
        assert (got["keys64"] == np.uint64(POISON64)).all() and got["won"] == 0
        return
    assert np.array_equal(got["keys64"], want["keys64"][band]), f"{what}: keys64"
    assert got["won"] == int(want["wins"][band].sum()), (what, got["won"], int(want["wins"][band].sum()))
    assert got["mask_stats"][COUNTED].tolist() == want["mask_stats"][COUNTED].tolist(), (what, got["mask_stats"].tolist(), want["mask_stats"].tolist())
    assert np.array_equal(got["depth"][band].view(np.uint32), want["depth"][band].view(np.uint32)), f"{what}: depth inside the band"
    outside = np.ones(h, bool)
    outside[band] = False
    assert np.array_equal(got["depth"][outside].view(np.uint32), before[outside].view(np.uint32)), f"{what}: depth outside the band"
