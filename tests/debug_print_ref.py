"""A numpy restatement of the reference's GPU debug print, for the tests (no GPU, no library):

  * the buffer and its slot rule (Shaders/DebugPrintCommon.hlsl): PrintChar takes slot = count++ and drops the entry when the slot is
    >= 4096; PrintString advances 8 pixels a character and stops at a zero code;
  * PrintLabel / PrintUInt and the one-thread stats printer (Shaders/GpuDebugPrintStats.hlsl), as written;
  * the draw (Shaders/GpuDebugPrint.hlsl and its blend state) in the pinned per-pixel form of DESIGN.md section 3.6, in float64:
    quad corners in fp32 (they decide coverage, so they are the kernel's own numbers), coverage min <= centre < max, UV =
    UvMin + (centre - min) / Size * (UvMax - UvMin), a bilinear tap at uv * size - 0.5 with clamp addressing, SRC_ALPHA /
    INV_SRC_ALPHA on the UNORM values with alpha ONE / ZERO, and one round-to-nearest to 8 bits per channel per entry.

composite() also carries the fp32 error bound of that formula through the entries (see fp32_delta) and returns, per byte, the
interval of values a correct fp32 evaluation may store.
"""
import numpy as np

MAX_ENTRIES = 4096
ADVANCE = 8
EPS = 2.0 ** -24  # unit roundoff of fp32


class Buffer:
    """count, then entries {x, y, code, color}; only the first min(count, 4096) entries are defined."""

    def __init__(self):
        self.count = 0
        self.entries = np.zeros((MAX_ENTRIES, 4), np.uint32)

    def words(self) -> np.ndarray:
        """The device layout: u32 count, then the entries."""
        return np.concatenate([np.array([self.count & 0xFFFFFFFF], np.uint32), self.entries.reshape(-1)])

    @property
    def used(self) -> int:
        return min(self.count, MAX_ENTRIES)


def print_char(buf: Buffer, x: int, y: int, code: int, color: int):
    index = buf.count
    buf.count += 1
    if index >= MAX_ENTRIES:
        return
    buf.entries[index] = (x & 0xFFFFFFFF, y & 0xFFFFFFFF, code & 0xFFFFFFFF, color & 0xFFFFFFFF)


def print_string(buf: Buffer, x: int, y: int, color: int, codes):
    """PrintString over any number of codes (the HLSL packs eight into two words): stops at a zero code."""
    for code in codes:
        if code == 0:
            return
        print_char(buf, x, y, code, color)
        x += ADVANCE


def print_label(buf: Buffer, x: int, y: int, color: int, label: str):
    assert len(label) == 8
    print_string(buf, x, y, color, [ord(c) & 0xFF for c in label])


def print_uint(buf: Buffer, x: int, y: int, value: int, color: int):
    divisor, started = 10000, False
    for i in range(5):
        digit = value // divisor
        value -= digit * divisor
        divisor = max(1, divisor // 10)
        if digit != 0 or started or i == 4:
            started = True
            print_char(buf, x, y, 48 + digit, color)
            x += ADVANCE


def print_stats(buf: Buffer, frustum: int, occlusion: int):
    color = 0xFFFFFFFF
    print_label(buf, 8, 20, color, "FRUSTUM ")
    print_uint(buf, 8 + 8 * 8, 20, frustum, color)
    print_label(buf, 8, 36, color, "OCCLUDE ")
    print_uint(buf, 8 + 8 * 8, 36, occlusion, color)


def print_text(buf: Buffer, x: int, y: int, color: int, text: bytes):
    print_string(buf, x, y, color, list(text))


# ---- the draw -------------------------------------------------------------------------------------------------------------------

def entry_quad(entry, glyphs, first_char: int, char_count: int):
    """(minx, miny, maxx, maxy) as fp32, or None when the entry draws nothing: a code outside [FirstChar, FirstChar + CharCount)
    (u32 arithmetic) or past the glyph table, or an empty / negative / NaN quad."""
    x, y, code = int(entry[0]), int(entry[1]), int(entry[2])
    if code < first_char or code >= ((first_char + char_count) & 0xFFFFFFFF) or code >= glyphs.shape[0]:
        return None
    g = glyphs[code].astype(np.float32)
    with np.errstate(all="ignore"):
        minx = np.float32(np.float32(x) + g[6])
        miny = np.float32(np.float32(y) + g[7])
        maxx = np.float32(minx + g[4])
        maxy = np.float32(miny + g[5])
    if not (minx < maxx and miny < maxy):
        return None
    return minx, miny, maxx, maxy


def covered_range(lo, hi, n):
    """Pixels p in [0, n) with lo <= p + 0.5 < hi, as a slice."""
    a = int(max(np.ceil(float(lo) - 0.5), 0))
    b = int(min(np.ceil(float(hi) - 0.5), n))
    return a, max(a, b)


def _round8(v):
    with np.errstate(invalid="ignore"):
        return np.floor(np.clip(np.nan_to_num(v, nan=0.0), 0.0, 1.0) * 255.0 + 0.5).astype(np.int64)


def _tap(atlas64, tx, ty):
    """Bilinear tap at texel-space positions (ty: (n, 1), tx: (1, m)), clamp addressing; also the largest step between adjacent
    texels, per axis, over the 4 x 4 window around the footprint (what a position error can move the tap across)."""
    ah, aw = atlas64.shape
    fx, fy = np.floor(tx), np.floor(ty)
    wx, wy = tx - fx, ty - fy
    ix, iy = fx.astype(np.int64), fy.astype(np.int64)
    cx = lambda i: np.clip(i, 0, aw - 1)
    cy = lambda i: np.clip(i, 0, ah - 1)
    T = lambda dx, dy: atlas64[cy(iy + dy), cx(ix + dx)]
    top = T(0, 0) + (T(1, 0) - T(0, 0)) * wx
    bot = T(0, 1) + (T(1, 1) - T(0, 1)) * wx
    gx = np.zeros(np.broadcast(tx, ty).shape)
    gy = np.zeros_like(gx)
    for dy in range(-1, 3):
        for dx in range(-1, 3):
            if dx < 2:
                gx = np.maximum(gx, np.abs(T(dx + 1, dy) - T(dx, dy)))
            if dy < 2:
                gy = np.maximum(gy, np.abs(T(dx, dy + 1) - T(dx, dy)))
    return top + (bot - top) * wy, gx, gy


def fp32_delta(glyph, aw, ah, gx, gy, ca, diff):
    """The fp32 error bound of the pinned formula for one entry (per pixel; `diff` = |Color - dst| per channel). eps = 2^-24.

    Per axis, with U = max(|UvMin|, |UvMax|) and A the atlas side: d = c - min, q = d / Size, duv = UvMax - UvMin, m = q duv and
    u = UvMin + m are five roundings of values no larger than U, so |du| <= 5 eps U; t = u A - 0.5 adds two roundings of values no
    larger than U A and the fraction t - floor(t) one of at most 1: |dt| <= 8 eps max(U A, 1). A floor that falls on the other side
    of an integer is the same bilinear surface (it is continuous), reached with the slope of the neighbouring cell: the tap moves by
    at most |dt_x| Gx + |dt_y| Gy, G the largest step between adjacent texels in the 4 x 4 window around the footprint. Four texels
    c / 255 and two levels of lerp (sub, mul, add on values <= 1) add 8 eps. alpha = Color.a * tap: ca itself and the product, 2 eps.
    out = Color a + dst (1 - a): the error of a enters as |Color - dst| da; Color / 255, dst / 255, 1 - a, two products and a sum are
    6 eps; the store v * 255 + 0.5 is two more roundings of values <= 256, 2 eps in UNORM units. Alpha channel: da + 2 eps."""
    ux = max(abs(float(glyph[0])), abs(float(glyph[2])))
    uy = max(abs(float(glyph[1])), abs(float(glyph[3])))
    dtx = 8.0 * EPS * max(ux * aw, 1.0)
    dty = 8.0 * EPS * max(uy * ah, 1.0)
    dtap = dtx * gx + dty * gy + 8.0 * EPS
    da = ca * dtap + 2.0 * EPS
    return diff * da[..., None] + 8.0 * EPS, da + 2.0 * EPS


def composite(image: np.ndarray, buf: Buffer, glyphs: np.ndarray, atlas: np.ndarray, first_char: int, char_count: int):
    """image: (H, W, 4) uint8 RGBA. Returns (out, lo, hi, covered): the float64 result rounded, the interval [lo, hi] of bytes an fp32
    evaluation within fp32_delta of it may hold (carried through the entries: blending is monotone in dst), and the covered mask."""
    H, W = image.shape[:2]
    out = image.astype(np.int64)
    lo, hi = out.copy(), out.copy()
    covered = np.zeros((H, W), bool)
    atlas64 = atlas.astype(np.float64) / 255.0
    ah, aw = atlas.shape
    for i in range(buf.used):
        e = buf.entries[i]
        q = entry_quad(e, glyphs, first_char, char_count)
        if q is None:
            continue
        minx, miny, maxx, maxy = q
        x0, x1 = covered_range(minx, maxx, W)
        y0, y1 = covered_range(miny, maxy, H)
        if x0 >= x1 or y0 >= y1:
            continue
        g = glyphs[int(e[2])].astype(np.float64)
        cx = np.arange(x0, x1)[None, :] + 0.5
        cy = np.arange(y0, y1)[:, None] + 0.5
        u = g[0] + (cx - float(minx)) / g[4] * (g[2] - g[0])
        v = g[1] + (cy - float(miny)) / g[5] * (g[3] - g[1])
        tap, gx, gy = _tap(atlas64, u * aw - 0.5, v * ah - 0.5)
        color = int(e[3])
        c = np.array([(color >> s) & 255 for s in (0, 8, 16)], np.float64) / 255.0
        ca = ((color >> 24) & 255) / 255.0
        a = ca * tap
        sl = (slice(y0, y1), slice(x0, x1))

        def blend(dst_bytes):
            d = dst_bytes[..., :3] / 255.0
            return c * a[..., None] + d * (1.0 - a[..., None]), np.abs(c - d)

        val, diff = blend(out[sl])
        out[sl] = np.concatenate([_round8(val), _round8(a)[..., None]], axis=-1)
        vlo, dlo = blend(lo[sl])
        vhi, dhi = blend(hi[sl])
        dc_lo, da = fp32_delta(g, aw, ah, gx, gy, ca, dlo)
        dc_hi, _ = fp32_delta(g, aw, ah, gx, gy, ca, dhi)
        # blending is monotone in dst (0 <= a <= 1): the two ends of [lo, hi], each widened by its own bound, span what fp32 may store
        new_lo = np.concatenate([_round8(np.minimum(vlo - dc_lo, vhi - dc_hi)), _round8(a - da)[..., None]], axis=-1)
        new_hi = np.concatenate([_round8(np.maximum(vlo + dc_lo, vhi + dc_hi)), _round8(a + da)[..., None]], axis=-1)
        lo[sl], hi[sl] = new_lo, new_hi
        covered[sl] = True
    return out.astype(np.uint8), lo.astype(np.uint8), hi.astype(np.uint8), covered


def pack_rgba(image_u8: np.ndarray) -> np.ndarray:
    """(H, W, 4) uint8 -> (H, W) uint32, R in the low byte."""
    return np.ascontiguousarray(image_u8).view(np.uint32)[..., 0]


def unpack_rgba(words: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(words.astype(np.uint32))[..., None].view(np.uint8)


def smooth_atlas(w: int, h: int, seed: int) -> np.ndarray:
    """A synthetic smooth R8 atlas: a few low-frequency waves, adjacent texels a few LSB apart."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    f = np.zeros((h, w))
    for _ in range(4):
        kx, ky, ph = rng.uniform(0.5, 2.0), rng.uniform(0.5, 2.0), rng.uniform(0, 6.28)
        f += np.sin(2 * np.pi * (kx * x / w + ky * y / h) + ph)
    f = (f - f.min()) / (f.max() - f.min())
    return np.round(f * 255.0).astype(np.uint8)


def ambiguous_share(lo, hi, covered) -> float:
    amb = (lo != hi).any(axis=-1) & covered
    return float(amb.sum()) / max(int(covered.sum()), 1)
