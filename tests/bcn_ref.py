"""The numpy restatement of DESIGN.md section 3.13: a BC1 / BC3 / BC5 texel is an RGBA8 code word, decoded from its 4 x 4 block by integer
arithmetic with truncating divisions (`//`), and a chain of levels is blocks, row-major, level behind level with no padding. Nothing here
comes from the library: tests/test_bcn_ref.py holds it to Pillow's decoder (tests/golden/bcn_pillow.npz) and holds the library's decoder
(csrc/bc_decode.h, through ur_host_bc_decode_level) to it.

`faults` plants one mistake at a time (tests/test_bcn_ref.py::test_planted_errors_change_bytes shows that the inputs can see each):
  "weights"   the 2/3 and 1/3 weights of the four-colour palette exchanged
  "no3"       the three-colour mode ignored (always four colours)
  "bc3mode"   BC3's colour block honouring c0 <= c1
  "bigendian" the 48 index bits of an alpha block read big-endian
  "pitch"     the block-row pitch taken as wk >> 2
  "texels"    the level offset counted in texels (wk * hk units instead of blocks)
"""
from __future__ import annotations

import numpy as np

BC1, BC1_SRGB, BC3, BC3_SRGB, BC5 = 71, 72, 77, 78, 83
FORMATS = (BC1, BC1_SRGB, BC3, BC3_SRGB, BC5)


def block_bytes(fmt: int) -> int:
    return 8 if fmt in (BC1, BC1_SRGB) else 16


def is_srgb(fmt: int) -> bool:
    return fmt in (29, BC1_SRGB, BC3_SRGB)


def level_size(size: int, k: int) -> int:
    return max(1, size >> min(k, 16))


def level_blocks(width: int, height: int, k: int, faults=()) -> int:
    wk, hk = level_size(width, k), level_size(height, k)
    if "texels" in faults:
        return wk * hk
    return ((wk + 3) >> 2) * ((hk + 3) >> 2)


def level_offset_bytes(fmt: int, width: int, height: int, d: int, faults=()) -> int:
    return sum(level_blocks(width, height, k, faults) for k in range(d)) * block_bytes(fmt)


def chain_bytes(fmt: int, width: int, height: int, mips: int) -> int:
    return level_offset_bytes(fmt, width, height, mips)


def _expand565(c):
    r, g, b = (c >> 11) & 31, (c >> 5) & 63, c & 31
    return np.stack([(r << 3) | (r >> 2), (g << 2) | (g >> 4), (b << 3) | (b >> 2)], -1)


def colour_blocks(blocks8: np.ndarray, force_four: bool, faults=()) -> np.ndarray:
    """(n, 8) uint8 colour blocks -> (n, 16, 4) uint8 RGBA, texel n at bits 2n of the index word."""
    b = blocks8.astype(np.int64)
    c0, c1 = b[:, 0] | (b[:, 1] << 8), b[:, 2] | (b[:, 3] << 8)
    idx_word = b[:, 4] | (b[:, 5] << 8) | (b[:, 6] << 16) | (b[:, 7] << 24)
    idx = (idx_word[:, None] >> (2 * np.arange(16))[None, :]) & 3
    p0, p1 = _expand565(c0), _expand565(c1)
    four = np.ones_like(c0, bool) if (force_four or "no3" in faults) else c0 > c1
    a, bb = (1, 2) if "weights" in faults else (2, 1)
    pal4 = np.stack([p0, p1, (a * p0 + bb * p1) // 3, (bb * p0 + a * p1) // 3], 1)  # (n, 4, 3)
    pal3 = np.stack([p0, p1, (p0 + p1) // 2, np.zeros_like(p0)], 1)
    pal = np.where(four[:, None, None], pal4, pal3)
    alpha = np.where(four[:, None], 255, np.array([255, 255, 255, 0])[None, :])  # (n, 4)
    rgb = np.take_along_axis(pal, idx[:, :, None].repeat(3, 2), 1)
    a8 = np.take_along_axis(alpha, idx, 1)
    return np.concatenate([rgb, a8[:, :, None]], -1).astype(np.uint8)


def alpha_blocks(blocks8: np.ndarray, faults=()) -> np.ndarray:
    """(n, 8) uint8 alpha-style blocks -> (n, 16) uint8, texel n at bits 3n of the little-endian 48-bit word."""
    b = blocks8.astype(np.int64)
    a0, a1 = b[:, 0], b[:, 1]
    order = range(5, -1, -1) if "bigendian" in faults else range(6)
    bits = sum(b[:, 2 + j] << (8 * i) for i, j in enumerate(order))
    idx = (bits[:, None] >> (3 * np.arange(16))[None, :]) & 7
    pal8 = [a0, a1] + [((8 - k) * a0 + (k - 1) * a1) // 7 for k in range(2, 8)]
    pal6 = [a0, a1] + [((6 - k) * a0 + (k - 1) * a1) // 5 for k in range(2, 6)] + [np.zeros_like(a0), np.full_like(a0, 255)]
    pal = np.where((a0 > a1)[:, None], np.stack(pal8, 1), np.stack(pal6, 1))
    return np.take_along_axis(pal, idx, 1).astype(np.uint8)


def decode_blocks(fmt: int, blocks: np.ndarray, faults=()) -> np.ndarray:
    """(n, 8 or 16) uint8 blocks -> (n, 16, 4) uint8 RGBA code words (the _SRGB formats give their UNORM twins' codes)."""
    blocks = np.ascontiguousarray(blocks, np.uint8).reshape(-1, block_bytes(fmt))
    if fmt in (BC1, BC1_SRGB):
        return colour_blocks(blocks, False, faults)
    if fmt in (BC3, BC3_SRGB):
        out = colour_blocks(blocks[:, 8:], "bc3mode" not in faults, faults)
        out[:, :, 3] = alpha_blocks(blocks[:, :8], faults)
        return out
    assert fmt == BC5, fmt
    out = np.zeros((blocks.shape[0], 16, 4), np.uint8)
    out[:, :, 0] = alpha_blocks(blocks[:, :8], faults)
    out[:, :, 1] = alpha_blocks(blocks[:, 8:], faults)
    out[:, :, 3] = 255
    return out


def decode_level(fmt: int, data, wk: int, hk: int, faults=()) -> np.ndarray:
    """The blocks of one level (bytes or uint8 array, at least the level's bytes) -> (hk, wk, 4) uint8."""
    per = block_bytes(fmt)
    data = np.frombuffer(bytes(data), np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.asarray(data, np.uint8).reshape(-1)
    across, down = (wk + 3) >> 2, (hk + 3) >> 2
    texels = decode_blocks(fmt, data[:across * down * per].reshape(-1, per), faults)  # (blocks, 16, 4)
    pitch = max(1, wk >> 2) if "pitch" in faults else across
    y, x = np.mgrid[0:hk, 0:wk]
    block = np.minimum((y >> 2) * pitch + (x >> 2), texels.shape[0] - 1)  # (a planted pitch or offset must not run out of the array)
    return texels[block, 4 * (y & 3) + (x & 3)]


def decode_chain(fmt: int, data, width: int, height: int, mips: int, faults=()) -> list[np.ndarray]:
    """A whole chain -> its levels as (hk, wk, 4) uint8 arrays: what an RGBA8 texture that holds the decoded texels is made of."""
    data = np.frombuffer(bytes(data), np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.asarray(data, np.uint8).reshape(-1)
    assert data.size == chain_bytes(fmt, width, height, mips), (data.size, chain_bytes(fmt, width, height, mips))
    out = []
    for k in range(mips):
        at = min(level_offset_bytes(fmt, width, height, k, faults), data.size - block_bytes(fmt))
        out.append(decode_level(fmt, data[at:], level_size(width, k), level_size(height, k), faults))
    return out


# ---- the inputs: every bit pattern is a valid block, so random bytes are textures

def structured_blocks(fmt: int) -> np.ndarray:
    """Equal endpoints, both orders of the endpoints with every index, and one index bit set at a time through all 32 / 48 index bits."""
    out = []
    ramp2 = int(sum((n & 3) << (2 * n) for n in range(16)))
    ramp3 = int(sum((n & 7) << (3 * n) for n in range(16)))

    def colour(c0, c1, idx):
        return np.frombuffer(int(c0 | (c1 << 16) | (idx << 32)).to_bytes(8, "little"), np.uint8)

    def alpha(a0, a1, idx):
        return np.frombuffer(int(a0 | (a1 << 8) | (idx << 16)).to_bytes(8, "little"), np.uint8)

    colours = [colour(c0, c1, ramp2) for c0, c1 in ((0xF800, 0x001F), (0x001F, 0xF800), (0x1234, 0x1234), (0, 0), (0xFFFF, 0xFFFF), (0x8410, 0x8411), (0x8411, 0x8410))]
    colours += [colour(c0, c1, 1 << bit) for bit in range(32) for c0, c1 in ((0xF81F, 0x07E0), (0x07E0, 0xF81F))]
    alphas = [alpha(a0, a1, ramp3) for a0, a1 in ((255, 0), (0, 255), (77, 77), (0, 0), (255, 255), (100, 101), (101, 100))]
    alphas += [alpha(a0, a1, 1 << bit) for bit in range(48) for a0, a1 in ((200, 13), (13, 200))]
    if fmt in (BC1, BC1_SRGB):
        return np.stack(colours)
    if fmt in (BC3, BC3_SRGB):
        n = max(len(colours), len(alphas))
        return np.stack([np.concatenate([alphas[k % len(alphas)], colours[k % len(colours)]]) for k in range(n)])
    return np.stack([np.concatenate([alphas[k], alphas[(k * 7 + 3) % len(alphas)]]) for k in range(len(alphas))])


def random_chain(fmt: int, width: int, height: int, mips: int, seed: int, punch_through: bool = False) -> np.ndarray:
    """Random blocks for a whole chain. punch_through (BC1): every other block gets c0 <= c1, so that index 3 is transparent black."""
    rng = np.random.default_rng(seed)
    data = rng.integers(0, 256, chain_bytes(fmt, width, height, mips), dtype=np.uint8)
    if punch_through and fmt in (BC1, BC1_SRGB):
        b = data.reshape(-1, 8)
        c = np.sort(b[::2, :4].copy().view(np.uint16).reshape(-1, 2), axis=1)  # c0 <= c1
        b[::2, :4] = c.view(np.uint8).reshape(-1, 4)
    return data
