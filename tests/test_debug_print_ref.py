"""Known answers for tests/debug_print_ref.py, derived by hand from Shaders/DebugPrintCommon.hlsl, GpuDebugPrintStats.hlsl and the
pinned per-pixel definitions of the draw. No GPU, no library."""
import numpy as np
import pytest

from tests import debug_print_ref as R


def _codes(buf):
    return [int(c) for c in buf.entries[:buf.used, 2]]


@pytest.mark.parametrize("value,want", [
    (0, "0"), (7, "7"), (120, "120"), (12345, "12345"), (99999, "99999"),
    (100000, ":0000"),  # 100000 / 10000 = 10: the first "digit" is 48 + 10 = 58, as the shader writes it
])
def test_print_uint(value, want):
    b = R.Buffer()
    R.print_uint(b, 72, 20, value, 0xFFFFFFFF)
    assert "".join(chr(c) for c in _codes(b)) == want
    assert _codes(b)[0] == ord(want[0])
    assert [int(x) for x in b.entries[:b.used, 0]] == [72 + 8 * i for i in range(len(want))]  # no gap for a suppressed zero
    assert all(int(y) == 20 for y in b.entries[:b.used, 1])


def test_print_uint_100000_first_code_is_58():
    b = R.Buffer()
    R.print_uint(b, 0, 0, 100000, 0)
    assert _codes(b)[0] == 58


def test_stats_printer_entries():
    """8 + 5 + 8 + 5 = 26 entries: the labels at x = 8 + 8 i, the numbers from x = 72, rows y = 20 and 36, colour 0xffffffff."""
    b = R.Buffer()
    R.print_stats(b, 12345, 67890)
    assert b.count == 26
    want = [(8 + 8 * i, 20, ord(c)) for i, c in enumerate("FRUSTUM ")] + [(72 + 8 * i, 20, ord(c)) for i, c in enumerate("12345")] \
        + [(8 + 8 * i, 36, ord(c)) for i, c in enumerate("OCCLUDE ")] + [(72 + 8 * i, 36, ord(c)) for i, c in enumerate("67890")]
    got = [tuple(int(v) for v in e[:3]) for e in b.entries[:26]]
    assert got == want
    assert all(int(e[3]) == 0xFFFFFFFF for e in b.entries[:26])
    # small counters: leading zeros suppressed, so fewer entries
    b = R.Buffer()
    R.print_stats(b, 0, 42)
    assert b.count == 8 + 1 + 8 + 2
    assert [tuple(int(v) for v in e[:3]) for e in b.entries[8:9]] == [(72, 20, 48)]
    assert [tuple(int(v) for v in e[:3]) for e in b.entries[17:19]] == [(72, 36, ord("4")), (80, 36, ord("2"))]


def test_slot_rule_drops_past_4096_and_keeps_counting():
    b = R.Buffer()
    R.print_text(b, 0, 0, 1, b"A" * 4090)
    R.print_text(b, 5, 7, 2, b"BCDEFGHIJK")
    assert b.count == 4100 and b.used == 4096
    assert [int(c) for c in b.entries[4090:, 2]] == [ord(c) for c in "BCDEFG"]
    assert int(b.entries[4095, 0]) == 5 + 8 * 5
    assert b.words().size == 1 + 4096 * 4 and int(b.words()[0]) == 4100


def test_print_string_stops_at_zero():
    b = R.Buffer()
    R.print_text(b, 3, 4, 9, b"AB\0CD")
    assert b.count == 2 and _codes(b) == [65, 66]


def _one_glyph(size, offset=(0.0, 0.0), uv=(0.0, 0.0, 1.0, 1.0)):
    g = np.zeros((66, 10), np.float32)
    g[65] = (uv[0], uv[1], uv[2], uv[3], size[0], size[1], offset[0], offset[1], 8.0, 0.0)
    return g


def test_coverage_rule_on_centres_and_borders():
    """min <= centre < max. A quad from 2.5 to 5.5 has its edges exactly on pixel centres: pixel 2 (centre 2.5) is in, pixel 5
    (centre 5.5) is out. A quad from 2 to 5 has its edges exactly on pixel borders: pixels 2, 3, 4."""
    atlas = np.full((1, 1), 255, np.uint8)
    img = np.zeros((8, 8, 4), np.uint8)
    for off, want in ((0.5, [2, 3, 4]), (0.0, [2, 3, 4]), (0.25, [2, 3, 4]), (0.75, [3, 4, 5])):
        b = R.Buffer()
        R.print_char(b, 2, 2, 65, 0xFFFFFFFF)
        out, lo, hi, cov = R.composite(img, b, _one_glyph((3.0, 3.0), (off, off)), atlas, 65, 1)
        assert sorted(set(np.nonzero(cov)[1])) == want and sorted(set(np.nonzero(cov)[0])) == want, off
        assert (out[cov] == 255).all() and (out[~cov] == 0).all()
    assert R.covered_range(np.float32(2.5), np.float32(5.5), 8) == (2, 5)
    assert R.covered_range(np.float32(2.0), np.float32(5.0), 8) == (2, 5)
    assert R.covered_range(np.float32(-3.0), np.float32(1.5), 8) == (0, 1)   # clipped at the left edge; centre 1.5 is out
    assert R.covered_range(np.float32(6.0), np.float32(20.0), 8) == (6, 8)


def test_degenerate_entries_draw_nothing():
    g = _one_glyph((3.0, 3.0))
    assert R.entry_quad((1, 1, 64, 0), g, 65, 1) is None and R.entry_quad((1, 1, 66, 0), g, 65, 1) is None  # outside the range
    assert R.entry_quad((1, 1, 65, 0), g, 65, 1) is not None
    assert R.entry_quad((1, 1, 65, 0), g[:65], 65, 1) is None                                                # past the table
    for size in ((0.0, 3.0), (3.0, -1.0), (np.nan, 3.0), (3.0, np.nan)):
        assert R.entry_quad((1, 1, 65, 0), _one_glyph(size), 65, 1) is None
    assert R.entry_quad((1, 1, 65, 0), _one_glyph((3.0, 3.0), (np.nan, 0.0)), 65, 1) is None
    assert R.entry_quad((1, 1, 65, 0), g, 60, 0xFFFFFFFF) is None  # FirstChar + CharCount wraps to 59: code >= 59


def test_one_blended_pixel_by_hand():
    """A 2 x 2 atlas {0, 255; 255, 255}, a quad of one pixel mapped onto the whole atlas: the pixel centre lands on uv (0.5, 0.5),
    t = 0.5 * 2 - 0.5 = 0.5, so the tap is the mean of the four texels, 0.75. Colour (255, 0, 102, 204) -> alpha = 0.8 * 0.75 = 0.6.
    Over dst (51, 255, 0): r = 1 * 0.6 + 0.2 * 0.4 = 0.68 -> 173.4 -> 173; g = 0 + 1 * 0.4 = 0.4 -> 102; b = 0.4 * 0.6 = 0.24 -> 61.2 -> 61;
    a = 0.6 -> 153."""
    atlas = np.array([[0, 255], [255, 255]], np.uint8)
    img = np.zeros((3, 3, 4), np.uint8)
    img[1, 1] = (51, 255, 0, 7)
    b = R.Buffer()
    R.print_char(b, 1, 1, 65, (204 << 24) | (102 << 16) | (0 << 8) | 255)
    out, lo, hi, cov = R.composite(img, b, _one_glyph((1.0, 1.0)), atlas, 65, 1)
    assert cov.sum() == 1 and cov[1, 1]
    assert tuple(out[1, 1]) == (173, 102, 61, 153)
    assert (lo[1, 1] == out[1, 1]).all() and (hi[1, 1] == out[1, 1]).all()  # far from a rounding boundary
    # a second entry on top blends with the ROUNDED bytes: opaque white at tap 1
    R.print_char(b, 1, 1, 65, 0x80FFFFFF)
    out2, _, _, _ = R.composite(img, b, _one_glyph((1.0, 1.0)), np.full((1, 1), 255, np.uint8), 65, 1)
    first = np.array([255, 102, 102, 204])  # entry one at tap 1: alpha 0.8 -> (1*.8+.2*.2, 0+1*.2, .4*.8, .8) = (.84, .2, .32, .8) -> 214, 51, 82, 204
    a2 = 128 / 255
    want = [int(np.floor((1.0 * a2 + (v / 255.0) * (1 - a2)) * 255 + 0.5)) for v in (214, 51, 82)] + [128]
    assert tuple(out2[1, 1]) == tuple(want), (out2[1, 1], want, first)
    assert R.pack_rgba(out2)[1, 1] == want[0] | (want[1] << 8) | (want[2] << 16) | (want[3] << 24)
    assert (R.unpack_rgba(R.pack_rgba(out2)) == out2).all()


def test_entry_order_matters():
    atlas = np.full((1, 1), 255, np.uint8)
    img = np.full((4, 4, 4), 40, np.uint8)
    g = _one_glyph((2.0, 2.0))
    b1, b2 = R.Buffer(), R.Buffer()
    for b, order in ((b1, (0x900000FF, 0x6000FF00)), (b2, (0x6000FF00, 0x900000FF))):
        for col in order:
            R.print_char(b, 1, 1, 65, col)
    o1 = R.composite(img, b1, g, atlas, 65, 1)[0]
    o2 = R.composite(img, b2, g, atlas, 65, 1)[0]
    assert not (o1 == o2).all() and o1[1, 1, 3] == 0x60 and o2[1, 1, 3] == 0x90


def test_smooth_atlas_is_smooth():
    a = R.smooth_atlas(64, 48, 3).astype(int)
    assert a.min() == 0 and a.max() == 255
    assert np.abs(np.diff(a, axis=0)).max() <= 24 and np.abs(np.diff(a, axis=1)).max() <= 24


@pytest.mark.parametrize("kind", ["builtin", "smooth"])
def test_few_covered_pixels_sit_on_a_rounding_boundary(kind, urlib):
    """The scenes the GPU test composites, on the CPU: the share of covered pixels whose float64 value lies within the fp32 bound of a
    rounding boundary (so that either byte is accepted) is under 1 %, and the accepted interval is never wider than two bytes."""
    from tests import debug_print_cases as K
    for seed in K.SEEDS:
        img, buf, glyphs, atlas, first, count = (K.scene_builtin if kind == "builtin" else K.scene_smooth)(seed)
        out, lo, hi, cov = R.composite(img, buf, glyphs, atlas, first, count)
        share = R.ambiguous_share(lo, hi, cov)
        print(kind, seed, "entries", buf.used, "covered", int(cov.sum()), "ambiguous share", share)
        assert cov.sum() > 3000
        assert share < 0.01, (kind, seed, share)
        assert ((hi.astype(int) - lo.astype(int)) <= 1).all() and (lo <= out).all() and (out <= hi).all()
        assert (out[~cov] == img[~cov]).all()
