"""The numpy restatement of DESIGN.md section 3.15: the texel of a transcode source - BC2, BC4 and BC7 beside section 3.13's BC1, BC3 and BC5 -
is an RGBA8 code word, and a transcoded chain is ur_texture2d's RGBA8 chain, level k max(1, w >> min(k, 16)) by the same of h, 4 bytes a
texel, tightly packed. tests/bcn_ref.py decodes the five formats of 3.13; nothing here comes from the library.
tests/test_texture_source_ref.py holds this file to Pillow's decoder (tests/golden/texture_source_pillow.npz) and the library's host
decoder (csrc/bc_wide_decode.h, through ur_host_texture_decode_level) to this file; the GPU tests hold ur_texture_transcode to it.

BC7 is restated from the rule's text: the mode table below is the rule's table, a block becomes its 128 bits, least significant first,
and every field is a sum of bits. The partition rows and the anchors are BPTC's public tables, packed as the library packs them (a
two-subset row is 16 bits, texel n at bit n; a three-subset row 32 bits, texel n at bits 2n); every entry is held by the fixture: a
mode-1 / mode-2 block per partition with distinct constant endpoints per subset shows its row, one with all index bits set its anchors.

`faults` plants one mistake at a time (tests/test_texture_source_ref.py::test_planted_errors_change_bytes shows the inputs see each):
  "pbit_above"   the p-bit placed above the stored bits
  "no_round"     the + 32 of the interpolation dropped
  "anchor15"     the anchor of subset 1 always texel 15
  "no_rotation"  the rotation ignored
  "no_index_selection"  mode 4's index selection ignored
  "no_replication"      an endpoint expanded as v << (8 - b) alone
  "swap3"        the three-subset rows 9 and 10 exchanged
  "bc2_shift"    BC2's alpha as a << 4
  "pitch"        the destination pitch of an odd-width level rounded up to an even number of texels
"""
from __future__ import annotations

import numpy as np

from tests import bcn_ref as R

BC2, BC2_SRGB, BC4, BC7, BC7_SRGB = 74, 75, 80, 98, 99
FORMATS = R.FORMATS + (BC2, BC2_SRGB, BC4, BC7, BC7_SRGB)

# mode: subsets, partition bits, rotation bits, index-selection bits, colour bits, alpha bits, p-bit per endpoint, p-bit per subset, index bits, second index bits
MODES = ((3, 4, 0, 0, 4, 0, 1, 0, 3, 0), (2, 6, 0, 0, 6, 0, 0, 1, 3, 0), (3, 6, 0, 0, 5, 0, 0, 0, 2, 0), (2, 6, 0, 0, 7, 0, 1, 0, 2, 0),
         (1, 0, 2, 1, 5, 6, 0, 0, 2, 3), (1, 0, 2, 0, 7, 8, 0, 0, 2, 2), (1, 0, 0, 0, 7, 7, 1, 0, 4, 0), (2, 6, 0, 0, 5, 5, 1, 0, 2, 0))
WEIGHTS = {2: np.array([0, 21, 43, 64]), 3: np.array([0, 9, 18, 27, 37, 46, 55, 64]),
           4: np.array([0, 4, 9, 13, 17, 21, 26, 30, 34, 38, 43, 47, 51, 55, 60, 64])}
PART2 = np.array([
    0xCCCC, 0x8888, 0xEEEE, 0xECC8, 0xC880, 0xFEEC, 0xFEC8, 0xEC80, 0xC800, 0xFFEC, 0xFE80, 0xE800, 0xFFE8, 0xFF00, 0xFFF0, 0xF000,
    0xF710, 0x008E, 0x7100, 0x08CE, 0x008C, 0x7310, 0x3100, 0x8CCE, 0x088C, 0x3110, 0x6666, 0x366C, 0x17E8, 0x0FF0, 0x718E, 0x399C,
    0xAAAA, 0xF0F0, 0x5A5A, 0x33CC, 0x3C3C, 0x55AA, 0x9696, 0xA55A, 0x73CE, 0x13C8, 0x324C, 0x3BDC, 0x6996, 0xC33C, 0x9966, 0x0660,
    0x0272, 0x04E4, 0x4E40, 0x2720, 0xC936, 0x936C, 0x39C6, 0x639C, 0x9336, 0x9CC6, 0x817E, 0xE718, 0xCCF0, 0x0FCC, 0x7744, 0xEE22], np.int64)
PART3 = np.array([
    0xAA685050, 0x6A5A5040, 0x5A5A4200, 0x5450A0A8, 0xA5A50000, 0xA0A05050, 0x5555A0A0, 0x5A5A5050, 0xAA550000, 0xAA555500, 0xAAAA5500,
    0x90909090, 0x94949494, 0xA4A4A4A4, 0xA9A59450, 0x2A0A4250, 0xA5945040, 0x0A425054, 0xA5A5A500, 0x55A0A0A0, 0xA8A85454, 0x6A6A4040,
    0xA4A45000, 0x1A1A0500, 0x0050A4A4, 0xAAA59090, 0x14696914, 0x69691400, 0xA08585A0, 0xAA821414, 0x50A4A450, 0x6A5A0200, 0xA9A58000,
    0x5090A0A8, 0xA8A09050, 0x24242424, 0x00AA5500, 0x24924924, 0x24499224, 0x50A50A50, 0x500AA550, 0xAAAA4444, 0x66660000, 0xA5A0A5A0,
    0x50A050A0, 0x69286928, 0x44AAAA44, 0x66666600, 0xAA444444, 0x54A854A8, 0x95809580, 0x96969600, 0xA85454A8, 0x80959580, 0xAA141414,
    0x96960000, 0xAAAA1414, 0xA05050A0, 0xA0A5A5A0, 0x96000000, 0x40804080, 0xA9A8A9A8, 0xAAAAAA44, 0x2A4A5254], np.int64)
ANCHOR2 = np.array([15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 2, 8, 2, 2, 8, 8, 15, 2, 8, 2, 2, 8, 8, 2, 2,
                    15, 15, 6, 8, 2, 8, 15, 15, 2, 8, 2, 2, 2, 15, 15, 6, 6, 2, 6, 8, 15, 15, 2, 2, 15, 15, 15, 15, 15, 2, 2, 15], np.int64)
ANCHOR3A = np.array([3, 3, 15, 15, 8, 3, 15, 15, 8, 8, 6, 6, 6, 5, 3, 3, 3, 3, 8, 15, 3, 3, 6, 10, 5, 8, 8, 6, 8, 5, 15, 15,
                     8, 15, 3, 5, 6, 10, 8, 15, 15, 3, 15, 5, 15, 15, 15, 15, 3, 15, 5, 5, 5, 8, 5, 10, 5, 10, 8, 13, 15, 12, 3, 3], np.int64)
ANCHOR3B = np.array([15, 8, 8, 3, 15, 15, 3, 8, 15, 15, 15, 15, 15, 15, 15, 8, 15, 8, 15, 3, 15, 8, 15, 8, 3, 15, 6, 10, 15, 15, 10, 8,
                     15, 3, 15, 10, 10, 8, 9, 10, 6, 15, 8, 15, 3, 6, 6, 8, 15, 3, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 3, 15, 15, 8], np.int64)


def block_bytes(fmt: int) -> int:
    return 8 if fmt in (R.BC1, R.BC1_SRGB, BC4) else 16


def is_srgb(fmt: int) -> bool:
    return fmt in (29, R.BC1_SRGB, R.BC3_SRGB, BC2_SRGB, BC7_SRGB)


level_size = R.level_size


def chain_bytes(fmt: int, width: int, height: int, mips: int) -> int:
    """Bytes of the source chain: 3.13's layout with this file's block sizes."""
    return sum(R.level_blocks(width, height, k) for k in range(mips)) * block_bytes(fmt)


def rgba8_chain_bytes(width: int, height: int, mips: int) -> int:
    return 4 * sum(level_size(width, k) * level_size(height, k) for k in range(mips))


def subset_rows(subsets: int, faults=()) -> np.ndarray:
    """(64, 16): the subset of texel n under partition p (all zero for one subset)."""
    n = np.arange(16)
    if subsets == 1:
        return np.zeros((64, 16), np.int64)
    if subsets == 2:
        return (PART2[:, None] >> n[None, :]) & 1
    rows = PART3.copy()
    if "swap3" in faults:
        rows[[9, 10]] = rows[[10, 9]]
    return (rows[:, None] >> (2 * n)[None, :]) & 3


def anchors(subsets: int, faults=()):
    """The anchor texel of subset 1 and of subset 2 per partition (-1 where the mode has no such subset)."""
    none = np.full(64, -1, np.int64)
    if subsets == 1:
        return none, none
    if subsets == 2:
        return (np.full(64, 15, np.int64) if "anchor15" in faults else ANCHOR2), none
    return (np.full(64, 15, np.int64) if "anchor15" in faults else ANCHOR3A), ANCHOR3B


def _field(bits, pos: int, n: int):
    """The n bits from `pos` on, least significant first, of every row of the (k, 128 + pad) bit array."""
    return (bits[:, pos:pos + n] << np.arange(n)[None, :]).sum(1) if n else np.zeros(bits.shape[0], np.int64)


def _field_at(bits, pos, width, most: int):
    """Per row and texel: `width` (k, 16) bits from `pos` (k, 16) on; `most` is the largest width."""
    rows = np.arange(bits.shape[0])[:, None]
    out = np.zeros((bits.shape[0], 16), np.int64)
    for j in range(most):
        out |= np.where(j < width, bits[rows, pos + j], 0) << j
    return out


def _bc7_mode(bits, m: int, faults=()):
    """The blocks (their bits, (k, 136)) that are all of mode m -> (k, 16, 4) codes."""
    subsets, pb, rb, isb, cb, ab, epb, spb, ib, ib2 = MODES[m]
    k, ne = bits.shape[0], 2 * subsets
    pos = m + 1
    part = _field(bits, pos, pb); pos += pb
    rot = _field(bits, pos, rb); pos += rb
    isel = _field(bits, pos, isb); pos += isb
    ends = np.zeros((k, ne, 4), np.int64)
    for c in range(3):
        for e in range(ne):
            ends[:, e, c] = _field(bits, pos, cb); pos += cb
    if ab:
        for e in range(ne):
            ends[:, e, 3] = _field(bits, pos, ab); pos += ab
    width = np.array([cb, cb, cb, ab])
    if epb or spb:
        for e in range(ne):
            p = _field(bits, pos + (e if epb else e // 2), 1)
            for c in range(4 if (epb and ab) else 3):
                ends[:, e, c] = (ends[:, e, c] | (p << width[c])) if "pbit_above" in faults else ((ends[:, e, c] << 1) | p)
        pos += ne if epb else subsets
        width = width + np.array([1, 1, 1, 1 if (epb and ab) else 0])
    for c in range(4 if ab else 3):
        b = int(width[c])
        ends[:, :, c] = (ends[:, :, c] << (8 - b)) | (0 if "no_replication" in faults else (ends[:, :, c] >> (2 * b - 8)))
    if not ab:
        ends[:, :, 3] = 255
    n = np.arange(16)[None, :]
    subset = subset_rows(subsets, faults)[part]  # (k, 16)
    a1, a2 = (a[part][:, None] for a in anchors(subsets, faults))
    anchor = (n == 0) | (n == a1) | (n == a2)
    before = (n > 0).astype(np.int64) + (n > a1) * (a1 >= 0) + (n > a2) * (a2 >= 0)
    first = _field_at(bits, pos + n * ib - before, ib - anchor, ib)
    pos += 16 * ib - subsets
    second = _field_at(bits, pos + n * ib2 - (n > 0), ib2 - (n == 0), ib2) if ib2 else first
    w1, w2 = WEIGHTS[ib][first], (WEIGHTS[ib2][second] if ib2 else WEIGHTS[ib][first])
    swap = (isel[:, None] == 1) & ("no_index_selection" not in faults)
    wc, wa = np.where(swap, w2, w1), np.where(swap, w1, w2)
    rows = np.arange(k)[:, None]
    e0, e1 = ends[rows, 2 * subset], ends[rows, 2 * subset + 1]  # (k, 16, 4)
    w = np.stack([wc, wc, wc, wa], -1)
    out = ((64 - w) * e0 + w * e1 + (0 if "no_round" in faults else 32)) >> 6
    if rb and "no_rotation" not in faults:
        for r in (1, 2, 3):
            sel = rot == r
            out[sel, :, r - 1], out[sel, :, 3] = out[sel, :, 3].copy(), out[sel, :, r - 1].copy()
    return out


def bc7_blocks(blocks16: np.ndarray, faults=()) -> np.ndarray:
    """(n, 16) uint8 BC7 blocks -> (n, 16, 4) uint8 RGBA. Byte 0 == 0 is the reserved mode: (0, 0, 0, 0) for all 16 texels."""
    blocks16 = np.ascontiguousarray(blocks16, np.uint8).reshape(-1, 16)
    bits = np.concatenate([np.unpackbits(blocks16, axis=1, bitorder="little"), np.zeros((blocks16.shape[0], 8), np.uint8)], 1).astype(np.int64)
    b0 = blocks16[:, 0].astype(np.int64)
    mode = np.full(b0.shape, 8, np.int64)
    for m in range(7, -1, -1):
        mode[(b0 >> m) & 1 == 1] = m  # the lowest set bit wins
    out = np.zeros((blocks16.shape[0], 16, 4), np.int64)
    for m in range(8):
        sel = mode == m
        if sel.any():
            out[sel] = _bc7_mode(bits[sel], m, faults)
    return out.astype(np.uint8)


def bc2_blocks(blocks16: np.ndarray, faults=()) -> np.ndarray:
    blocks16 = np.ascontiguousarray(blocks16, np.uint8).reshape(-1, 16)
    out = R.colour_blocks(blocks16[:, 8:], True)
    a = blocks16[:, :8].astype(np.int64)
    nib = np.stack([a & 15, a >> 4], -1).reshape(-1, 16)  # texel n at bits 4n
    out[:, :, 3] = (nib << 4) if "bc2_shift" in faults else nib * 17
    return out


def bc4_blocks(blocks8: np.ndarray) -> np.ndarray:
    blocks8 = np.ascontiguousarray(blocks8, np.uint8).reshape(-1, 8)
    out = np.zeros((blocks8.shape[0], 16, 4), np.uint8)
    out[:, :, 0] = R.alpha_blocks(blocks8)
    out[:, :, 3] = 255
    return out


def decode_blocks(fmt: int, blocks, faults=()) -> np.ndarray:
    """(n, 8 or 16) uint8 blocks -> (n, 16, 4) uint8 RGBA code words (the _SRGB forms give their UNORM twins' codes)."""
    blocks = np.ascontiguousarray(blocks, np.uint8).reshape(-1, block_bytes(fmt))
    if fmt in R.FORMATS:
        return R.decode_blocks(fmt, blocks)
    if fmt in (BC2, BC2_SRGB):
        return bc2_blocks(blocks, faults)
    if fmt == BC4:
        return bc4_blocks(blocks)
    assert fmt in (BC7, BC7_SRGB), fmt
    return bc7_blocks(blocks, faults)


def _bytes(data) -> np.ndarray:
    return np.frombuffer(bytes(data), np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.asarray(data, np.uint8).reshape(-1)


def decode_level(fmt: int, data, wk: int, hk: int, faults=()) -> np.ndarray:
    """The blocks of one level (bytes or uint8 array, at least the level's bytes) -> (hk, wk, 4) uint8."""
    per = block_bytes(fmt)
    across, down = (wk + 3) >> 2, (hk + 3) >> 2
    texels = decode_blocks(fmt, _bytes(data)[:across * down * per], faults)
    y, x = np.mgrid[0:hk, 0:wk]
    return texels[(y >> 2) * across + (x >> 2), 4 * (y & 3) + (x & 3)]


def decode_chain(fmt: int, data, width: int, height: int, mips: int, faults=()) -> list:
    """A whole source chain -> its levels as (hk, wk, 4) uint8 arrays."""
    data = _bytes(data)
    assert data.size == chain_bytes(fmt, width, height, mips), (data.size, chain_bytes(fmt, width, height, mips))
    out, at = [], 0
    for k in range(mips):
        out.append(decode_level(fmt, data[at:], level_size(width, k), level_size(height, k), faults))
        at += R.level_blocks(width, height, k) * block_bytes(fmt)
    return out


def pack_rgba8(levels, faults=()) -> np.ndarray:
    """Levels -> the bytes of ur_texture2d's RGBA8 chain: rows of 4 wk bytes, level behind level, no padding."""
    if "pitch" not in faults:
        return np.concatenate([np.ascontiguousarray(a).reshape(-1) for a in levels])
    out = np.zeros(sum(a.size for a in levels), np.uint8)
    at = 0
    for a in levels:
        hk, wk = a.shape[:2]
        pitch = 4 * (wk + (wk & 1))
        for y in range(hk):
            lo = at + y * pitch
            row = a[y].reshape(-1)[:max(0, min(4 * wk, at + a.size - lo))]
            out[lo:lo + row.size] = row
        at += a.size
    return out


def transcode_chain(fmt: int, data, width: int, height: int, mips: int, faults=()) -> np.ndarray:
    """What ur_texture_transcode writes: the bytes of the RGBA8 chain of the decoded source chain."""
    out = pack_rgba8(decode_chain(fmt, data, width, height, mips, faults), faults)
    assert out.size == rgba8_chain_bytes(width, height, mips)
    return out


# ---- the inputs

def bc7_block(mode: int, partition=0, rotation=0, index_selection=0, endpoints=(), pbits=(), indices=(0,) * 16, indices2=(0,) * 16) -> np.ndarray:
    """A BC7 block from its fields. endpoints: 2 x subsets stored (r, g, b[, a]) tuples; pbits: one per endpoint or per subset as the mode has
    them; indices / indices2: 16 primary / secondary indices, an anchor's below half the range."""
    subsets, pb, rb, isb, cb, ab, epb, spb, ib, ib2 = MODES[mode]
    v, pos = 1 << mode, mode + 1

    def put(val, n):
        nonlocal v, pos
        assert 0 <= val < (1 << n), (val, n)
        v |= int(val) << pos
        pos += n

    put(partition, pb), put(rotation, rb), put(index_selection, isb)
    assert len(endpoints) == 2 * subsets and len(pbits) == (2 * subsets if epb else (subsets if spb else 0))
    for c in range(3):
        for e in endpoints:
            put(e[c], cb)
    if ab:
        for e in endpoints:
            put(e[3], ab)
    for p in pbits:
        put(p, 1)
    a1, a2 = (int(a[partition]) for a in anchors(subsets))
    for n in range(16):
        put(indices[n], ib - (n in (0, a1, a2)))
    if ib2:
        for n in range(16):
            put(indices2[n], ib2 - (n == 0))
    assert pos == 128, pos
    return np.frombuffer(v.to_bytes(16, "little"), np.uint8)


def force_modes(blocks16: np.ndarray) -> np.ndarray:
    """Random BC7 blocks get the mode bits of mode (row mod 8): plain random bytes are mode 0 half the time and mode 7 once in 256."""
    b = np.array(blocks16, np.uint8).reshape(-1, 16)
    m = np.arange(b.shape[0]) % 8
    b[:, 0] = (b[:, 0] & ~((2 << m) - 1) & 255) | (1 << m)
    return b


def _rand_ends(rng, mode):
    subsets, _, _, _, cb, ab, epb, spb, _, _ = MODES[mode]
    ends = [tuple(int(rng.integers(0, 1 << cb)) for _ in range(3)) + ((int(rng.integers(0, 1 << ab)),) if ab else ()) for _ in range(2 * subsets)]
    return ends, [int(rng.integers(0, 2)) for _ in range(2 * subsets if epb else (subsets if spb else 0))]


def structured_blocks(fmt: int) -> np.ndarray:
    """BC7: per partitioned mode and partition, distinct constant endpoints per subset under zero indices (the row) and the far endpoints
    under all index bits set (the anchors); every rotation with both index selections in mode 4 and every rotation in mode 5 over random
    endpoints and ramps of indices; one index bit set at a time in every mode; four reserved-mode blocks (byte 0 == 0) at the end.
    BC2: BC3's colour blocks behind every nibble value, and one alpha bit at a time. BC4: 3.13's alpha blocks."""
    if fmt in (BC2, BC2_SRGB):
        colours = R.structured_blocks(R.BC1)
        alphas = [np.frombuffer(int(sum(((n + s) & 15) << (4 * n) for n in range(16))).to_bytes(8, "little"), np.uint8) for s in range(16)]
        alphas += [np.frombuffer(int(1 << bit).to_bytes(8, "little"), np.uint8) for bit in range(64)]
        return np.stack([np.concatenate([alphas[k % len(alphas)], colours[k % len(colours)]]) for k in range(max(len(colours), len(alphas)))])
    if fmt == BC4:
        return R.structured_blocks(R.BC5)[:, :8].copy()
    assert fmt in (BC7, BC7_SRGB)
    rng = np.random.default_rng(0xBC7)
    out = []
    for mode in (0, 1, 2, 3, 7):
        subsets, pb, _, _, cb, ab, epb, spb, ib, _ = MODES[mode]
        top = (1 << cb) - 1
        npb = 2 * subsets if epb else (subsets if spb else 0)
        for p in range(1 << pb):
            flat = [((s * top) // (subsets - 1),) * 3 + ((top,) if ab else ()) for s in range(subsets) for _ in range(2)]
            out.append(bc7_block(mode, p, endpoints=flat, pbits=[0] * npb))
            far = [((e & 1) * top,) * 3 + (((e & 1) * top,) if ab else ()) for e in range(2 * subsets)]
            a1, a2 = (int(a[p]) for a in anchors(subsets))
            ones = [(1 << (ib - (n in (0, a1, a2)))) - 1 for n in range(16)]
            out.append(bc7_block(mode, p, endpoints=far, pbits=[1] * npb, indices=ones))
    ramp = lambda bits, s: [((n + s) % (1 << (bits - (n == 0)))) if n == 0 else (n * 5 + s) % (1 << bits) for n in range(16)]  # noqa: E731
    for rot in range(4):
        for isel in range(2):
            ends, _ = _rand_ends(rng, 4)
            out.append(bc7_block(4, rotation=rot, index_selection=isel, endpoints=ends, indices=ramp(2, rot), indices2=ramp(3, isel + 2)))
        ends, _ = _rand_ends(rng, 5)
        out.append(bc7_block(5, rotation=rot, endpoints=ends, indices=ramp(2, rot + 1), indices2=ramp(2, rot + 2)))
    for mode in range(8):
        ends, pbits = _rand_ends(rng, mode)
        base = bc7_block(mode, int(rng.integers(0, 1 << MODES[mode][1])) if MODES[mode][1] else 0, endpoints=ends, pbits=pbits)
        index_bits = 16 * (MODES[mode][8] + MODES[mode][9]) - MODES[mode][0] - (1 if MODES[mode][9] else 0)
        for bit in range(128 - index_bits, 128):
            b = base.copy()
            b[bit >> 3] |= 1 << (bit & 7)
            out.append(b)
    out += [np.frombuffer(bytes([0]) + bytes(rng.integers(0, 256, 15, dtype=np.uint8)), np.uint8) for _ in range(3)] + [np.zeros(16, np.uint8)]
    return np.stack(out)


def random_chain(fmt: int, width: int, height: int, mips: int, seed: int) -> np.ndarray:
    """Random blocks for a whole source chain; BC7 chains cycle through the eight modes block by block."""
    if fmt in R.FORMATS:
        return R.random_chain(fmt, width, height, mips, seed, punch_through=True)
    data = np.random.default_rng(seed).integers(0, 256, chain_bytes(fmt, width, height, mips), dtype=np.uint8)
    return force_modes(data).reshape(-1) if fmt in (BC7, BC7_SRGB) else data
