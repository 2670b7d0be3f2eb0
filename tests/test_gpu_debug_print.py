"""GpuDebugPrint on the MI355X: the entries the stats and text kernels write equal the restatement's bit for bit, and the composite
equals the float64 restatement (tests/debug_print_ref.py) up to the fp32 error bound of the pinned formula.

The bound (debug_print_ref.fp32_delta, derived there from the operation count): per entry the tap position carries at most
8 eps max(U A, 1) texels of error per axis (U the largest |UV| of the glyph, A the atlas side, eps = 2^-24), which moves the tap by at
most that times the largest step between adjacent texels around the footprint; plus 8 eps for the texel conversions and lerps, 2 eps
for alpha, 6 eps for the blend and 2 eps for the store. A byte is right if it is a round-to-nearest of some value within that bound of
the float64 result: the restatement carries the interval [lo, hi] of such bytes through the entries. Pixels whose interval is wider
than one byte may take either; tests/test_debug_print_ref.py shows on the CPU that they are under 1 % of the covered pixels of these
scenes. Every pixel no entry covers must be byte-equal to the input."""
import numpy as np
import pytest

from tests import debug_print_cases as K
from tests import debug_print_ref as R

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _words(t):
    return t.cpu().numpy().view(np.uint32)


def _draw(hotpath, img, buf_words, glyphs, atlas, first, count, bands=1):
    """Composite on the device; the image as `bands` equal row bands, each its own call on its own tensor."""
    torch = _torch()
    from unclerenderer_amd.hotpath import to_device
    h, w = img.shape[:2]
    d_buf, d_gl, d_at = to_device(buf_words), to_device(np.ascontiguousarray(glyphs, np.float32)), torch.from_numpy(np.ascontiguousarray(atlas)).cuda()
    packed = R.pack_rgba(img)
    rows = h // bands
    out = []
    for r in range(bands):
        band = to_device(np.ascontiguousarray(packed[r * rows:(r + 1) * rows]))
        hotpath.debug_print_draw(d_buf, d_gl, d_at, band, w, h, r * rows, rows, first_char=first, char_count=count)
        out.append(band)
    torch.cuda.synchronize()
    return R.unpack_rgba(np.concatenate([_words(b) for b in out]))


def _check(got, img, buf, glyphs, atlas, first, count, share=False):
    out, lo, hi, cov = R.composite(img, buf, glyphs, atlas, first, count)
    assert (got[~cov] == img[~cov]).all(), "a pixel no entry covers changed"
    bad = (got < lo) | (got > hi)
    exact = (got == out)
    print("covered", int(cov.sum()), "bytes off the float64 rounding", int((~exact).sum()), "outside the interval", int(bad.sum()),
          "ambiguous share", R.ambiguous_share(lo, hi, cov))
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:5], got[bad][:5], lo[bad][:5], hi[bad][:5])
    if share:  # (the scenes whose share the CPU test has shown from the restatement alone)
        assert R.ambiguous_share(lo, hi, cov) < 0.01
    return out, cov


def test_entries_bit_for_bit(hotpath):
    torch = _torch()
    from unclerenderer_amd.hotpath import debug_print_buffer, to_device
    ref, buf = R.Buffer(), debug_print_buffer()
    buf.fill_(0x5A5A5A5A)
    stats = torch.full((2,), 77, dtype=torch.int32, device="cuda")
    hotpath.debug_print_reset(buf, stats)
    torch.cuda.synchronize()
    assert int(_words(buf)[0]) == 0 and _words(stats).tolist() == [0, 0] and int(_words(buf)[1]) == 0x5A5A5A5A  # only the count word
    buf.zero_()

    def stats_line(a, b):
        hotpath.debug_print_stats(to_device(np.array([a, b], np.uint32)), buf)
        R.print_stats(ref, a, b)

    def text(x, y, s, color):
        hotpath.debug_print_text(buf, x, y, s, color)
        R.print_text(ref, x, y, color, s)

    stats_line(0, 7)
    stats_line(120, 12345)
    stats_line(99999, 100000)
    stats_line(4294967295, 65536)
    text(3, 400, b"HELLO, WORLD", 0x80FF8040)
    text(9, 9, b"ENDS\0HERE", 0x11223344)             # stops at the zero code
    text(0, 0, b"\0", 1)
    text(0xFFFFFFF8, 5, b"WRAP", 0xFFFFFFFF)           # x + 8 i in u32
    text(1, 2, bytes(32 + (i % 64) for i in range(700)), 0xCAFEF00D)  # three launches
    torch.cuda.synchronize()
    assert np.array_equal(_words(buf), ref.words())
    # past 4096: entries dropped, the count still counting - across a chunk, a stats print and single characters
    text(5, 6, bytes(33 + (i % 60) for i in range(3200)), 0x01020304)
    assert ref.count < 4096
    stats_line(31, 4)
    text(7, 8, bytes(40 + (i % 50) for i in range(400)), 0x0A0B0C0D)  # crosses 4096 inside a launch
    assert ref.count > 4096
    stats_line(5, 6)
    text(1, 1, b"LATE", 0xFFFFFFFF)
    torch.cuda.synchronize()
    got = _words(buf)
    assert int(got[0]) == ref.count and ref.count > 4096
    assert np.array_equal(got, ref.words())


@pytest.mark.parametrize("kind", ["builtin", "smooth"])
def test_composite_matches_restatement(hotpath, kind):
    for seed in K.SEEDS:
        img, buf, glyphs, atlas, first, count = (K.scene_builtin if kind == "builtin" else K.scene_smooth)(seed)
        got = _draw(hotpath, img, buf.words(), glyphs, atlas, first, count)
        _check(got, img, buf, glyphs, atlas, first, count, share=True)


def test_stats_lines_with_builtin_font(hotpath):
    """The two lines the frame draws, printed and composited on the device."""
    torch = _torch()
    from unclerenderer_amd.hotpath import debug_print_buffer, to_device
    atlas, glyphs, first, count = K.builtin_font()
    img = K.background(5)
    buf = debug_print_buffer()
    hotpath.debug_print_stats(to_device(np.array([2718, 31415], np.uint32)), buf)
    band = to_device(R.pack_rgba(img))
    hotpath.debug_print_draw(buf, to_device(glyphs), torch.from_numpy(atlas).cuda(), band, K.W, K.H, first_char=first, char_count=count)
    torch.cuda.synchronize()
    ref = R.Buffer()
    R.print_stats(ref, 2718, 31415)
    assert np.array_equal(_words(buf), ref.words())
    out, cov = _check(R.unpack_rgba(_words(band)), img, ref, glyphs, atlas, first, count)
    assert (R.unpack_rgba(_words(band)) == out).all()  # opaque white on texel centres: exact
    lit = (out == 255).all(axis=-1) & cov
    assert lit[13:20, 8:104].any() and lit[29:36, 8:112].any() and cov[13:21, 8:104].all() and cov[29:37, 8:112].all()
    assert cov.sum() == 8 * 8 * (12 + 13)


def test_entry_order(hotpath):
    """Overlapping entries of different colours and alphas come out in entry order; two entries swapped give the swapped result."""
    atlas, glyphs, first, count = K.smooth_font(4)
    img = K.background(9)
    a, b = R.Buffer(), R.Buffer()
    cols = (0xC02040FF, 0x70FF3010, 0xFF10E0A0, 0x3300FFFF)
    for buf, order in ((a, (0, 1, 2, 3)), (b, (0, 2, 1, 3))):
        for k in order:
            R.print_string(buf, 60 + 3 * k, 58 + 2 * k, cols[k], b"OVERLAP@TILE")
    ga = _draw(hotpath, img, a.words(), glyphs, atlas, first, count)
    gb = _draw(hotpath, img, b.words(), glyphs, atlas, first, count)
    oa, _ = _check(ga, img, a, glyphs, atlas, first, count)
    ob, _ = _check(gb, img, b, glyphs, atlas, first, count)
    assert (oa != ob).any() and (ga != gb).any()
    differ = (oa.astype(int) - ob.astype(int))
    assert np.abs(differ).max() > 8  # the order is visible, far beyond a rounding
    assert np.abs(ga.astype(int) - gb.astype(int)).max() > 8


def test_skipped_and_degenerate_entries(hotpath):
    atlas, glyphs, first, count = K.builtin_font()
    img = K.background(3)
    g = glyphs.copy()
    g = np.concatenate([g, np.zeros((32, 10), np.float32)])  # codes 96..127 in the table, outside the font's range
    g[96] = g[65]
    g[40, 4] = 0.0       # '(' empty
    g[41, 5] = -8.0      # ')' negative
    g[42, 4] = np.nan    # '*' NaN size
    g[43, 6] = np.nan    # '+' NaN offset
    buf = R.Buffer()
    R.print_string(buf, 20, 30, 0xFFFFFFFF, bytes([96, 31, 200, 255, 40, 41, 42, 43]))   # none of these draws
    R.print_char(buf, 30, 60, 1 << 20, 0xFFFFFFFF)                                          # a code far past the table
    nothing = _draw(hotpath, img, buf.words(), g, atlas, first, count)
    assert (nothing == img).all()
    R.print_string(buf, 100, 100, 0xFF00FF00, b"OK")
    got = _draw(hotpath, img, buf.words(), g, atlas, first, count)
    out, cov = _check(got, img, buf, g, atlas, first, count)
    assert cov.sum() == 128 and (got == out).all()
    # FirstChar / CharCount of the caller decide: the same buffer with the range moved past 'O' and 'K'
    assert (_draw(hotpath, img, buf.words(), g, atlas, 90, 6) == img).all()
    # a glyph table shorter than the range: codes past it draw nothing
    assert (_draw(hotpath, img, buf.words(), g[:70], atlas, first, count) == img).all()
    # an empty buffer, and a count far past 4096 with 4096 undrawable entries
    assert (_draw(hotpath, img, R.Buffer().words(), g, atlas, first, count) == img).all()
    big = R.Buffer()
    big.count = 1 << 31
    assert (_draw(hotpath, img, big.words(), g, atlas, first, count) == img).all()


def test_clipping_tiles_and_bands(hotpath):
    """Quads hanging over each image edge are clipped; text across the 64-pixel tile borders and the band borders comes out whole;
    2, 3 and 8 bands give the unsplit image's bytes."""
    for kind in ("builtin", "smooth"):
        atlas, glyphs, first, count = K.builtin_font() if kind == "builtin" else K.smooth_font(6)
        img = K.background(17)
        buf = R.Buffer()
        col = 0xE0FFFFFF if kind == "builtin" else 0xB040C0FF
        R.print_string(buf, 0, 0, col, b"TOP EDGE")                      # y - 7 < 0
        R.print_string(buf, K.W - 20, 40, col, b"RIGHT")                 # runs off the right edge
        R.print_string(buf, 30, K.H + 3, col, b"BOTTOM")                 # hangs over the bottom edge
        R.print_string(buf, 0xFFFFFFFC, 90, col, b"LEFT")                # x wraps: (float)x is 2^32, off-screen
        glyphs = glyphs.copy()
        glyphs[64, 6] = -3.0                                             # '@' with a negative x Offset ...
        at_left = buf.count
        R.print_string(buf, 0, 120, col, b"@@")                          # ... at x = 0 hangs over the left edge
        R.print_string(buf, 36, 67, col, b"ACROSS THE TILE BORDER")      # x = 64 and y = 64 inside the glyphs
        R.print_string(buf, 120, 130, col, b"X=128")
        for y in (76, 52, 100, 22, 40, 58, 94, 112, 130):                # rows 72; 48, 96; 18, 36, ... inside the glyph cells
            R.print_string(buf, 4 + y, y, col ^ (y << 8), b"BAND BORDER")
        whole = _draw(hotpath, img, buf.words(), glyphs, atlas, first, count)
        out, cov = _check(whole, img, buf, glyphs, atlas, first, count)
        assert R.entry_quad(buf.entries[at_left], glyphs, first, count)[0] == -3.0
        assert cov[0].any() and cov[-1].any() and cov[:, -1].any() and cov[:, 0].any() and cov[63:65, 63:65].all() and cov[71:73].any()
        for bands in (2, 3, 8):
            assert (_draw(hotpath, img, buf.words(), glyphs, atlas, first, count, bands=bands) == whole).all(), (kind, bands)


def test_full_buffer(hotpath):
    """4096 entries (and a count beyond): every one is drawn, in order, across many tiles."""
    atlas, glyphs, first, count = K.builtin_font()
    rng = np.random.default_rng(8)
    img = K.background(21, 512, 288)
    buf = R.Buffer()
    while buf.count < 4200:
        R.print_string(buf, int(rng.integers(0, 500)), int(rng.integers(0, 290)), int(rng.integers(0, 1 << 32)) | 0xFF000000,
                       bytes(int(c) for c in rng.integers(33, 96, 16)))
    got = _draw(hotpath, img, buf.words(), glyphs, atlas, first, count)
    out, cov = _check(got, img, buf, glyphs, atlas, first, count)
    assert (got == out).all()  # opaque colours on texel centres: exact
    assert (_draw(hotpath, img, buf.words(), glyphs, atlas, first, count, bands=4) == got).all()
