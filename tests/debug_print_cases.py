"""Seeded scenes for the GpuDebugPrint composite tests: a random background, a font and a buffer of entries. Built on the CPU, so that
tests/test_debug_print_ref.py can show from the restatement alone that few covered pixels sit within the fp32 bound of a rounding
boundary, and tests/test_gpu_debug_print.py can run the same scenes through the kernel."""
import numpy as np

from tests import debug_print_ref as R

W, H = 200, 144  # not a multiple of the 64 x 64 tile; 144 rows split into 2, 3 and 8 equal bands


def background(seed, w=W, h=H):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)


def builtin_font():
    from unclerenderer_amd import hostmath
    atlas, glyphs, first, count = hostmath.debug_font()
    return atlas, glyphs, first, count


def smooth_font(seed):
    """A 96 x 80 smooth atlas and glyphs for codes 32..127 with fractional sizes and offsets and sub-texel UV rectangles."""
    rng = np.random.default_rng(seed)
    atlas = R.smooth_atlas(96, 80, seed)
    glyphs = np.zeros((128, 10), np.float32)
    for code in range(32, 128):
        u0, v0 = rng.uniform(0.0, 0.7, 2)
        du, dv = rng.uniform(0.05, 0.3, 2)
        glyphs[code] = (u0, v0, u0 + du, v0 + dv, rng.uniform(5.0, 14.0), rng.uniform(6.0, 18.0), rng.uniform(-3.0, 3.0), rng.uniform(-12.0, 2.0), 8.0, 0.0)
    return atlas, glyphs, 32, 96


def random_text(seed, first, count, strings=24, w=W, h=H, opaque_share=0.0):
    """`strings` strings of 3..20 random codes of the font at random positions (some hanging over every edge), random colours;
    `opaque_share` of them with alpha 255."""
    rng = np.random.default_rng(seed)
    buf = R.Buffer()
    for s in range(strings):
        n = int(rng.integers(3, 21))
        codes = bytes(int(c) for c in rng.integers(first, first + count, n))
        x, y = int(rng.integers(0, w + 8)) - 12, int(rng.integers(0, h + 16)) - 4
        color = int(rng.integers(0, 1 << 32))
        if rng.random() < opaque_share:
            color |= 0xFF000000
        # positions are u32 in the buffer: a negative start wraps, as a shader printing at such a position would
        R.print_string(buf, max(x, 0), max(y, 0), color, codes)
    return buf


def scene_builtin(seed):
    atlas, glyphs, first, count = builtin_font()
    return background(seed), random_text(seed + 1, first, count, strings=30, opaque_share=0.5), glyphs, atlas, first, count


def scene_smooth(seed):
    atlas, glyphs, first, count = smooth_font(seed + 2)
    return background(seed), random_text(seed + 3, first, count, strings=30), glyphs, atlas, first, count


SEEDS = (11, 23)
