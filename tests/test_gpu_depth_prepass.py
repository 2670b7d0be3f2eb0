"""ur_depth_prepass on the GPU: the target is byte-equal to the fp32 path of tests/depth_ref.py (the raster rule of DESIGN.md section
3.8), and so are stats6 except [3], which is structural (large triangles that found no room in the queue)."""
import numpy as np
import pytest

from tests import depth_ref as R
from tests.depth_gpu import DeviceDraws, run
from tests.test_depth_ref import H as HAND_H
from tests.test_depth_ref import W as HAND_W
from tests.test_depth_ref import hand_cases, soup_reference

pytestmark = pytest.mark.gpu

COUNTED = [0, 1, 2, 4, 5]


def _same(got, want, what):
    g, e = got.view(np.uint32), want.view(np.uint32)
    if not np.array_equal(g, e):
        bad = np.argwhere(g != e)
        y, x = bad[0]
        raise AssertionError(f"{what}: {bad.shape[0]} texels differ, first at (x {x}, y {y}): got {got[y, x]!r} ({g[y, x]:#010x}), want {want[y, x]!r} ({e[y, x]:#010x})")


@pytest.mark.parametrize("flags", [0, R.QUANTIZE_D24])
@pytest.mark.parametrize("name", sorted(hand_cases()))
def test_hand_cases(hotpath, name, flags):
    draws, stats = hand_cases()[name]
    cam = R.hand_camera(HAND_W, HAND_H)
    want, want_stats = R.depth_prepass(draws, *cam, HAND_W, HAND_H, flags=flags)
    assert tuple(int(v) for v in want_stats) == stats
    got, got_stats = run(hotpath, DeviceDraws(draws), *cam, HAND_W, HAND_H, flags=flags)
    _same(got, want, name)
    assert got_stats[COUNTED].tolist() == want_stats[COUNTED].tolist(), name


def test_command_level_cases(hotpath):
    """Another index format, a stride below 12, an index outside the view, InstanceCount 0, an empty command list."""
    import torch
    from tests.test_depth_ref import CORNER, _draw
    a, b, c, d = _draw([CORNER, CORNER]), _draw([CORNER]), _draw([CORNER, CORNER]), _draw([CORNER])
    a.index_format, b.stride, d.instance_count = 57, 8, 0
    c.indices, c.index_count = c.indices[:5], 6
    draws = [a, b, c, d]
    cam = R.hand_camera(HAND_W, HAND_H)
    want, want_stats = R.depth_prepass(draws, *cam, HAND_W, HAND_H)
    assert want_stats.tolist() == [1, 4, 0, 0, 0, 0]
    got, got_stats = run(hotpath, DeviceDraws(draws), *cam, HAND_W, HAND_H)
    _same(got, want, "command-level cases")
    assert got_stats.tolist() == [1, 4, 0, 0, 0, 0]
    m = torch.full((5, 3), 7.0, dtype=torch.float32, device="cuda")
    hotpath.depth_prepass(*cam, None, m, command_count=0)
    torch.cuda.synchronize()
    assert (m.cpu().numpy() == 0.0).all()


@pytest.mark.parametrize("dirty", [False, True])
@pytest.mark.parametrize("w,h,seed", R.SOUPS)
def test_soups(hotpath, w, h, seed, dirty):
    """With the queue, with a queue of one entry (every large triangle overflows: stats[3] > 0) and without one; the second run of each
    is the same bytes; the last on a target misaligned by 4 bytes (the head and tail of the clear)."""
    draws, view, proj, want, want_stats, info, _ = soup_reference(w, h, R.DIRTY_SEED if dirty else seed, dirty)
    dd = DeviceDraws(draws)
    large = info["large"] > 0
    try:
        for reserve in (1 << 16, 1, 0):
            hotpath.raster_reserve(reserve)
            got, got_stats = run(hotpath, dd, view, proj, w, h, offset_floats=1 if reserve == 0 else 0)
            _same(got, want, f"soup {w}x{h}, reserve {reserve}")
            assert got_stats[COUNTED].tolist() == want_stats[COUNTED].tolist()
            assert (got_stats[3] == 0) if (reserve == 1 << 16 or not large) else (got_stats[3] > 0), (reserve, got_stats.tolist())
            again, again_stats = run(hotpath, dd, view, proj, w, h)
            assert np.array_equal(again.view(np.uint32), got.view(np.uint32)) and np.array_equal(again_stats, got_stats), "two runs differ"
    finally:
        hotpath.raster_reserve(0)


@pytest.mark.parametrize("w,h,seed", R.SOUPS[:2])
def test_soups_d24(hotpath, w, h, seed):
    from unclerenderer_amd import synth
    draws, view, proj, plain, want_stats, _, _ = soup_reference(w, h, seed)
    want, _ = R.depth_prepass(draws, view, proj, w, h, flags=R.QUANTIZE_D24)
    assert np.array_equal(want.view(np.uint32), synth.quantize_d24(plain).view(np.uint32))
    hotpath.raster_reserve(4096)
    try:
        got, got_stats = run(hotpath, DeviceDraws(draws), view, proj, w, h, flags=R.QUANTIZE_D24)
    finally:
        hotpath.raster_reserve(0)
    _same(got, want, f"D24 soup {w}x{h}")
    assert got_stats[COUNTED].tolist() == want_stats[COUNTED].tolist()


class _NoCommands:
    commands = None  # with ranges the slots come from the ranges' own command buffer


def test_selections(hotpath):
    """All slots, a list with an index base, ranges with an empty range and a count below the range size - against the restatement
    under the same selection; an empty list leaves the target all 0.0."""
    import torch
    from unclerenderer_amd.hotpath import to_device
    w, h = 64, 64
    draws = R.soup(w, h, 7, triangles=600)
    draws[1].instance_count = 1
    n = len(draws)
    dd = DeviceDraws(draws)
    view, proj = R.soup_camera(w, h)
    ref = lambda slots: R.depth_prepass(draws, view, proj, w, h, slots=slots)  # noqa: E731

    want, ws = ref(None)
    got, gs = run(hotpath, dd, view, proj, w, h)
    _same(got, want, "every slot")
    assert gs[COUNTED].tolist() == ws[COUNTED].tolist()

    base = 1000
    idx = np.array([base + 4, base + 0, base + 2, base + 1, base + 3], np.uint32)  # (the last two lie behind the count)
    for count in (3, 0):
        slots = R.selected_slots(n, visible=(idx, count), index_base=base)
        assert slots == [4, 0, 2][:count]
        want, ws = ref(slots)
        got, gs = run(hotpath, dd, view, proj, w, h, visible=(to_device(idx), to_device(np.array([count], np.uint32))), index_base=base)
        _same(got, want, f"list of {count}")
        assert gs[COUNTED].tolist() == ws[COUNTED].tolist()
        if count == 0:
            assert (got == 0.0).all() and not gs.any()

    offsets, counts = np.array([0, 2, 2, 5], np.uint32), np.array([1, 0, 3], np.uint32)
    slots = R.selected_slots(n, ranges=(offsets, counts))
    assert slots == [0, 2, 3, 4]
    want, ws = ref(slots)
    compacted = torch.from_numpy(dd.host_commands.view(np.int32).copy()).to("cuda")
    got, gs = run(hotpath, _NoCommands(), view, proj, w, h, ranges=(to_device(offsets), compacted, to_device(counts)))
    _same(got, want, "ranges")
    assert gs[COUNTED].tolist() == ws[COUNTED].tolist()
