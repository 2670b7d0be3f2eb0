"""ur_gbuffer_pass_materials, ur_gbuffer_pass_masked and ur_forward_pass held directly to the float64 ray caster (tests/raycast_tex.py) on
its scenes of connected meshes with analytic textures: which texels are compared and how closely is that file's, the same that
tests/test_raycast_tex.py applies to the restatements. Every pass runs over the depth ur_depth_prepass wrote for the opaque selection in
the same stream.

No run uploads the ramps as BC3: an exact encoding of a ramp block does not exist. A block of a ramp with slopes (bx, by) holds up to
seven codes per channel (a + bx i + by j, i, j = 0..3), and a BC3 colour block has four palette entries; with by = 0 the four codes
a, a + bx, a + 2 bx, a + 3 bx would need the endpoints a and a + 3 bx, both expansions of 5- or 6-bit values, in every block of a row of 16
blocks - the 5-bit expansions are 8 or 9 apart, so 3 bx would be a multiple of about 8.25 and the row would span more than 255 codes.
(The alpha block's eight entries (k c1 + (7 - k) c0) / 7 could hold a + 2 k exactly; the colour block cannot.)"""
import numpy as np
import pytest

from tests import forward_gpu
from tests import gbuffer_mask_gpu
from tests import raycast_ref as R
from tests import raycast_tex as T
from tests.gbuffer_gpu import device_draws, run
from tests.gbuffer_tex_gpu import device_materials
from tests.test_raycast_ref import report

pytestmark = pytest.mark.gpu


def uploaded(sc):
    dd = device_draws(sc.draws)
    return dd, device_materials(T.ref_materials(sc.mats)), gbuffer_mask_gpu.Selections(dd, sc.opaque, list(sc.masked))


def prepass(hotpath, sc, sel, w, h):
    """The depth ur_depth_prepass writes for the opaque selection: a (h, w) float32 device tensor."""
    import torch
    depth = torch.full((h, w), float("nan"), dtype=torch.float32, device="cuda")
    hotpath.depth_prepass(sc.view, sc.proj, sel.call_commands, depth, **sel.opaque)
    return depth


def gbuffer(hotpath, sc, w, h):
    """(the G-buffer kernel's dict over the prepass' depth - ur_gbuffer_pass_masked's with a masked selection -, that depth)."""
    dd, mats, sel = uploaded(sc)
    depth = prepass(hotpath, sc, sel, w, h)
    if sc.masked:
        return gbuffer_mask_gpu.run(hotpath, sel, mats, sc.view, sc.proj, depth.cpu().numpy(), w, h), depth.cpu().numpy()
    return run(hotpath, dd, sc.view, sc.proj, depth, w, h, materials=mats), depth.cpu().numpy()


def held(record_property, what, sc, rc, got, depth):
    compared = T.classify(rc)[0]
    res = T.compare_masked(rc, got, sc.draws, sc.masked, compared) if sc.masked else T.compare_gbuffer(rc, got, sc.draws, compared)
    if not sc.masked:
        res.update(T.compare_depth(rc, depth, compared))
    if sc.name == "levels":
        res.update(T.compare_levels(rc, got, compared))
    report(record_property, what, res)
    assert R.failures(res) == 0, (what, res)


@pytest.mark.parametrize("w,h", R.TARGETS)
@pytest.mark.parametrize("name", ["textured", "levels", "masked"])
def test_gbuffer(hotpath, record_property, name, w, h):
    sc, rc = T.cast_scene(name, w, h)
    got, depth = gbuffer(hotpath, sc, w, h)
    kernel = "ur_gbuffer_pass_masked" if sc.masked else "ur_gbuffer_pass_materials"
    held(record_property, f"ur_depth_prepass + {kernel}, {name} {w}x{h}", sc, rc, got, depth)


@pytest.mark.parametrize("w,h", R.TARGETS)
def test_textured_strip_with_and_without_the_queue(hotpath, record_property, w, h):
    """uv and tangent through the near clip: the strip's cut triangles and the two target-spanning ones, through the large-triangle queue
    and, with no queue, through the wave that found them."""
    sc, rc = T.cast_scene("textured strip", w, h)
    try:
        for reserve in (1 << 12, 0):
            hotpath.raster_reserve(reserve)
            got, depth = gbuffer(hotpath, sc, w, h)
            held(record_property, f"ur_depth_prepass + ur_gbuffer_pass_materials, textured strip {w}x{h}, queue of {reserve}", sc, rc, got, depth)
    finally:
        hotpath.raster_reserve(0)


@pytest.mark.parametrize("w,h", R.TARGETS)
@pytest.mark.parametrize("name", T.FORWARD_SCENES)
def test_forward(hotpath, record_property, name, w, h):
    sc, rc = T.cast_scene(name, w, h)
    _, mats, sel = uploaded(sc)
    depth = prepass(hotpath, sc, sel, w, h).cpu().numpy()
    before = T.background(w, h)
    got = forward_gpu.run(hotpath, sel, mats, sc.view, sc.proj, depth, w, h, forward_gpu.DeviceFrame(hotpath, T.scene_frame(sc)), before, masked=bool(sc.masked))
    compared = T.classify(rc, forward=True)[0]
    res = T.compare_forward(rc, got["hdr"], before, compared)
    res.update(T.compare_depth(rc, got["depth"], compared))
    if sc.masked:
        least = int((compared & rc["hit"][0] & np.isin(rc["draw"][0], list(sc.masked))).sum())
        bad = not least <= got["won"] <= least + int((~compared).sum())
        res["won"] = (int(bad), np.inf if bad else 0.0)
    report(record_property, f"ur_depth_prepass + ur_forward_pass, {name} {w}x{h}", res)
    assert R.failures(res) == 0, res
