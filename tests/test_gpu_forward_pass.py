"""ur_forward_pass on the GPU: hdr, keys, keys64, depth, won and both stats6 (except [3], structural) are byte-equal to
tests/forward_ref.py, the rule of DESIGN.md section 3.12; NaN is compared by NaN-ness, and a texel no key covers keeps its bytes."""
import numpy as np
import pytest

from tests import depth_ref as D
from tests import forward_ref as FW
from tests import gbuffer_ref as G
from tests.forward_gpu import DeviceFrame, run, same_forward, same_half
from tests.gbuffer_gpu import device_draws
from tests.gbuffer_mask_gpu import Selections
from tests.gbuffer_tex_gpu import device_materials
from tests.test_forward_ref import H as HAND_H
from tests.test_forward_ref import W as HAND_W
from tests.test_forward_ref import background, forward_soup, hand_cases, run_case

pytestmark = pytest.mark.gpu

_DEVICE = {}


def _background(w, h):
    return np.random.default_rng(w * 1000 + h).integers(0, 0x7800, (h, w, 4)).astype(np.uint16)


def _soup(hotpath, w, h, seed):
    """The soup's inputs and its device copy (draws, materials, range selections, the frame's tables), uploaded once."""
    key = (w, h, seed)
    ref = forward_soup(w, h, seed)
    if key not in _DEVICE:
        draws, mats, opaque, masked, *_, frm, _ = ref
        dd = device_draws(draws)
        _DEVICE[key] = (dd, device_materials(mats), Selections(dd, [s for _, s in opaque], [s for _, s in masked]), DeviceFrame(hotpath, frm))
    return ref, _DEVICE[key]


def _want(ref, w, h, **kw):
    draws, mats, opaque, masked, view, proj, depth, frm, _ = ref
    args = dict(materials=mats, select=opaque, mask_select=masked, hdr=_background(w, h))
    args.update(kw)
    depth = args.pop("depth", depth)
    frm = args.pop("frame", frm)
    return FW.forward_pass(draws, view, proj, depth, w, h, frm, **args)


_WANT = {}


def _soup_want(ref, w, h):
    """The textured, masked whole-frame reference over the seeded background: computed once per soup and left unchanged."""
    if (w, h) not in _WANT:
        _WANT[(w, h)] = _want(ref, w, h)
    return _WANT[(w, h)]


@pytest.mark.parametrize("name", sorted(hand_cases()))
def test_hand_cases(hotpath, name):
    draws, mats, opaque, masked, frm = hand_cases()[name]
    want, depth, _ = run_case(name)
    dd = device_draws(draws)
    got = run(hotpath, Selections(dd, opaque, masked), device_materials(mats), *D.hand_camera(HAND_W, HAND_H), depth, HAND_W, HAND_H, DeviceFrame(hotpath, frm), background())
    same_forward(got, want, depth, name)


@pytest.mark.parametrize("textured", [True, False])
@pytest.mark.parametrize("w,h,seed", FW.SOUPS)
def test_soups(hotpath, w, h, seed, textured):
    """Textured and untextured (materials == NULL: key 0 everywhere, nothing discarded), with room in the large-triangle queue and without a queue."""
    ref, (_, mats, sel, dframe) = _soup(hotpath, w, h, seed)
    depth = ref[6]
    want = _soup_want(ref, w, h) if textured else _want(ref, w, h, materials=None)
    try:
        for reserve in (1 << 16, 0):
            hotpath.raster_reserve(reserve)
            got = run(hotpath, sel, mats if textured else None, ref[4], ref[5], depth, w, h, dframe, _background(w, h))
            same_forward(got, want, depth, f"soup {w}x{h}, textured {textured}, reserve {reserve}")
    finally:
        hotpath.raster_reserve(0)


def test_soup_d24(hotpath):
    w, h, seed = FW.SOUPS[0]
    ref, (_, mats, sel, dframe) = _soup(hotpath, w, h, seed)
    draws, _, opaque, _, view, proj, *_ = ref
    depth, _ = D.depth_prepass(draws, view, proj, w, h, flags=D.QUANTIZE_D24, slots=[s for _, s in opaque])
    want = _want(ref, w, h, depth=depth, flags=G.QUANTIZE_D24)
    got = run(hotpath, sel, mats, view, proj, depth, w, h, dframe, _background(w, h), flags=G.QUANTIZE_D24)
    same_forward(got, want, depth, "D24 soup")


def test_selection_kinds_and_uncovered_texels(hotpath):
    """Ranges are the other tests'. Visible lists of a few slots in another order than the slots', with an index base: the resolve finds a
    masked key's slot through keys64, and the texels no key covers keep the background's bytes. Every slot without a mask: the keys are
    ur_gbuffer_pass_materials', and depth is not written."""
    import torch
    from unclerenderer_amd.hotpath import gbuffer_targets, raster_draws
    w, h, seed = FW.SOUPS[0]
    ref, (dd, mats, _, dframe) = _soup(hotpath, w, h, seed)
    draws, _, opaque, masked, view, proj, *_ = ref
    o_slots, m_slots = [opaque[k][1] for k in (4, 0, 2)], [masked[k][1] for k in (3, 0)]
    depth, _ = D.depth_prepass(draws, view, proj, w, h, slots=o_slots)
    want = _want(ref, w, h, depth=depth, select=list(enumerate(o_slots)), mask_select=list(enumerate(m_slots)))
    covered = want["keys"] != 0
    assert 0 < covered.sum() < w * h and want["won"] > 0 and np.array_equal(want["hdr"][~covered], _background(w, h)[~covered])
    got = run(hotpath, Selections(dd, o_slots, m_slots, "lists", index_base=1000), mats, view, proj, depth, w, h, dframe, _background(w, h))
    same_forward(got, want, depth, "lists")
    assert np.array_equal(got["hdr"][~covered], _background(w, h)[~covered])

    sel = Selections(dd, [], [], "lists")
    sel.opaque, sel.call_commands = {}, dd.commands
    depth, _ = D.depth_prepass(draws, view, proj, w, h)
    want = _want(ref, w, h, depth=depth, select=None, mask_select=None)
    got = run(hotpath, sel, mats, view, proj, depth, w, h, dframe, _background(w, h), masked=False)
    same_forward(got, want, depth, "every slot, mask == NULL", masked=False)
    half = lambda: torch.full((h, w, 4), float("nan"), dtype=torch.float16, device="cuda")  # noqa: E731
    word = lambda: torch.full((h, w), 0x5A5A5A5A, dtype=torch.int32, device="cuda")  # noqa: E731
    keys = word()
    hotpath.gbuffer_pass(view, proj, dd.commands, torch.from_numpy(depth.copy()).to("cuda"), gbuffer_targets(half(), half(), word(), half(), keys), w, h, materials=mats)
    torch.cuda.synchronize()
    assert np.array_equal(got["keys"], keys.cpu().numpy().view(np.uint32))
    assert raster_draws(dd.commands).command_count == len(draws)


@pytest.mark.parametrize("bands", [((0, 65), (65, 65)), ((0, 37), (37, 41), (78, 52))])
def test_bands_against_the_whole_frame(hotpath, bands):
    """257 x 130 in bands: every band's hdr, keys, keys64 and depth rows are the whole frame's."""
    w, h, seed = FW.SOUPS[1]
    ref, (_, mats, sel, dframe) = _soup(hotpath, w, h, seed)
    depth, want = ref[6], _soup_want(ref, w, h)
    hotpath.raster_reserve(4096)
    try:
        for row0, rows in bands:
            got = run(hotpath, sel, mats, ref[4], ref[5], depth, w, h, dframe, _background(w, h), row0, rows)
            same_forward(got, want, depth, f"rows [{row0}, {row0 + rows})", row0, rows)
    finally:
        hotpath.raster_reserve(0)


def test_parts_and_determinism(hotpath):
    """The raster part, then the resolve part, leave the one call's bytes; the raster part alone leaves hdr as it was; a second run of the
    one call leaves the first one's bytes."""
    from unclerenderer_amd import lib
    w, h, seed = FW.SOUPS[1]
    ref, (_, mats, sel, dframe) = _soup(hotpath, w, h, seed)
    depth, want, bg = ref[6], _soup_want(ref, w, h), _background(w, h)
    common = (hotpath, sel, mats, ref[4], ref[5], depth, w, h, dframe, bg)
    first, second = run(*common), run(*common)
    apart = run(*common, parts_sequence=(lib.UR_GBUFFER_PART_RASTER, lib.UR_GBUFFER_PART_RESOLVE))
    raster_only = run(*common, parts_sequence=(lib.UR_GBUFFER_PART_RASTER,))
    same_forward(first, want, depth, "one call")
    same_forward(apart, want, depth, "raster part, then resolve part")
    assert first["won"] == second["won"] and not same_half(first["hdr"], second["hdr"]).any()
    for k in ("keys", "keys64"):
        assert np.array_equal(first[k], second[k]), k
    assert np.array_equal(first["depth"].view(np.uint32), second["depth"].view(np.uint32))
    assert np.array_equal(raster_only["keys"], want["keys"]) and np.array_equal(raster_only["hdr"], bg)


def test_small_lut_and_shadow_map(hotpath):
    """An 8 x 4 LUT and a 2 x 2 shadow map: every LUT tap clamps or sits next to a clamp, every shadow tap touches the border."""
    from dataclasses import replace
    from unclerenderer_amd import synth
    w, h, seed = FW.SOUPS[0]
    ref, (_, mats, sel, _) = _soup(hotpath, w, h, seed)
    frm = replace(ref[7], lut=synth.brdf_lut_procedural(8, 4), shadow=np.array([[0.3, 0.7], [0.9, 0.5]], np.float32))
    want = _want(ref, w, h, frame=frm)
    got = run(hotpath, sel, mats, ref[4], ref[5], ref[6], w, h, DeviceFrame(hotpath, frm), _background(w, h))
    same_forward(got, want, ref[6], "8 x 4 LUT, 2 x 2 shadow map")
    assert same_half(want["hdr"], _soup_want(ref, w, h)["hdr"]).any()  # (the tables matter)
