"""ur_shadow_map on the GPU: the map is byte-equal to the fp32 path of tests/shadow_ref.py (the raster rule of DESIGN.md section 3.7),
and so are stats4[0:3]; stats4[3] is structural (large triangles that found no room in the queue)."""
import numpy as np
import pytest

from tests import shadow_ref as R
from tests.shadow_gpu import DeviceDraws, run
from tests.test_shadow_ref import hand_cases

pytestmark = pytest.mark.gpu

_REF = {}


def _soup(w, h, seed):
    """The soup and its reference, computed once and left unchanged."""
    key = (w, h, seed)
    if key not in _REF:
        draws = R.soup(w, h, seed)
        m, s = R.shadow_map(draws, R.target_lvp(), w, h)
        m.setflags(write=False)
        _REF[key] = (draws, m, s)
    return _REF[key]


def _same(got, want, what):
    g, e = got.view(np.uint32), want.view(np.uint32)
    if not np.array_equal(g, e):
        bad = np.argwhere(g != e)
        y, x = bad[0]
        raise AssertionError(f"{what}: {bad.shape[0]} texels differ, first at (x {x}, y {y}): got {got[y, x]!r} ({g[y, x]:#010x}), want {want[y, x]!r} ({e[y, x]:#010x})")


@pytest.mark.parametrize("name", sorted(hand_cases()))
def test_hand_cases(hotpath, name):
    draws, stats = hand_cases()[name]
    want, want_stats = R.shadow_map(draws, R.target_lvp(), 8, 8)
    assert tuple(int(v) for v in want_stats) == stats
    got, got_stats = run(hotpath, DeviceDraws(draws), R.target_lvp(), 8, 8)
    _same(got, want, name)
    assert got_stats[:3].tolist() == want_stats.tolist(), name


def test_command_level_cases(hotpath):
    """Another index format, a stride below 12, an index outside the view, InstanceCount 0, an empty command list."""
    from tests.test_shadow_ref import CORNER, ON_CENTRE, _draw
    a, b, c, d = _draw([CORNER, ON_CENTRE]), _draw([CORNER]), _draw([CORNER, CORNER]), _draw([CORNER])
    a.index_format, b.stride, d.instance_count = 57, 8, 0
    c.indices, c.index_count = c.indices[:5], 6
    draws = [a, b, c, d]
    want, want_stats = R.shadow_map(draws, R.target_lvp(), 8, 8)
    assert want_stats.tolist() == [1, 4, 0]
    got, got_stats = run(hotpath, DeviceDraws(draws), R.target_lvp(), 8, 8)
    _same(got, want, "command-level cases")
    assert got_stats[:3].tolist() == [1, 4, 0]
    import torch
    m = torch.zeros((5, 3), dtype=torch.float32, device="cuda")
    hotpath.shadow_map(R.target_lvp(), None, m, command_count=0)
    torch.cuda.synchronize()
    assert (m.cpu().numpy() == 1.0).all()


@pytest.mark.parametrize("w,h,seed", [(64, 64, 1), (257, 130, 2)])
def test_soups_small_targets(hotpath, w, h, seed):
    draws, want, want_stats = _soup(w, h, seed)
    dd = DeviceDraws(draws)
    for reserve in (4096, 0):
        hotpath.raster_reserve(reserve)
        got, got_stats = run(hotpath, dd, R.target_lvp(), w, h)
        _same(got, want, f"soup {w}x{h}, reserve {reserve}")
        assert got_stats[:3].tolist() == want_stats.tolist()
        again, again_stats = run(hotpath, dd, R.target_lvp(), w, h)
        assert np.array_equal(again.view(np.uint32), got.view(np.uint32)) and np.array_equal(again_stats, got_stats), "two runs differ"
    hotpath.raster_reserve(0)


def test_soup_2048_with_and_without_a_reserve(hotpath):
    w = h = 2048
    draws, want, want_stats = _soup(w, h, 3)
    dd = DeviceDraws(draws)
    hotpath.raster_reserve(1 << 20)
    got, got_stats = run(hotpath, dd, R.target_lvp(), w, h)
    _same(got, want, "soup 2048x2048 with a reserve")
    assert got_stats.tolist() == want_stats.tolist() + [0]
    hotpath.raster_reserve(0)
    got0, got0_stats = run(hotpath, dd, R.target_lvp(), w, h)
    _same(got0, want, "soup 2048x2048 without a reserve")
    assert got0_stats[:3].tolist() == want_stats.tolist() and got0_stats[3] > 0
    # a queue that overflows half way: the same bytes again
    hotpath.raster_reserve(3000)
    got1, got1_stats = run(hotpath, dd, R.target_lvp(), w, h)
    _same(got1, want, "soup 2048x2048 with a queue that overflows")
    assert 0 < got1_stats[3] <= got0_stats[3]
    hotpath.raster_reserve(0)


def test_selections(hotpath):
    """All slots, a list with an index base, ranges with an empty range and a count below the range size - against the restatement
    under the same selection; an empty list leaves the map all 1.0."""
    import torch
    from unclerenderer_amd.hotpath import to_device
    w, h = 64, 64
    draws = R.soup(w, h, 7, triangles=600)
    draws[1].instance_count = 1
    n = len(draws)
    dd = DeviceDraws(draws)
    lvp = R.target_lvp()
    ref = lambda slots: R.shadow_map(draws, lvp, w, h, slots=slots)  # noqa: E731

    want, ws = ref(None)
    got, gs = run(hotpath, dd, lvp, w, h)
    _same(got, want, "every slot")
    assert gs[:3].tolist() == ws.tolist()

    base = 1000
    idx = np.array([base + 4, base + 0, base + 2, base + 1, base + 3], np.uint32)  # (the last two lie behind the count)
    for count in (3, 0):
        slots = R.selected_slots(n, visible=(idx, count), index_base=base)
        assert slots == [4, 0, 2][:count]
        want, ws = ref(slots)
        got, gs = run(hotpath, dd, lvp, w, h, visible=(to_device(idx), to_device(np.array([count], np.uint32))), index_base=base)
        _same(got, want, f"list of {count}")
        assert gs[:3].tolist() == ws.tolist()
        if count == 0:
            assert (got == 1.0).all() and not gs.any()

    # ranges over a compacted copy: range 0 = slots [0, 2) with 1 drawn, range 1 empty, range 2 = slots [2, 5) with 3 drawn
    offsets, counts = np.array([0, 2, 2, 5], np.uint32), np.array([1, 0, 3], np.uint32)
    slots = R.selected_slots(n, ranges=(offsets, counts))
    assert slots == [0, 2, 3, 4]
    want, ws = ref(slots)
    compacted = torch.from_numpy(dd.host_commands.view(np.int32).copy()).to("cuda")
    got, gs = run(hotpath, _NoCommands(), lvp, w, h, ranges=(to_device(offsets), compacted, to_device(counts)))
    _same(got, want, "ranges")
    assert gs[:3].tolist() == ws.tolist()


class _NoCommands:
    commands = None  # with ranges the slots come from the ranges' own command buffer
