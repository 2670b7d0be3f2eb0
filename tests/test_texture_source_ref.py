"""DESIGN.md section 3.15 without a GPU: the numpy restatement (tests/texture_source_ref.py) against Pillow's decoder on the fixture
tests/golden/texture_source_pillow.npz and against hand-worked blocks, the library's host decoder (csrc/bc_wide_decode.h through
ur_host_texture_decode_level) against the restatement on the fixture and on whole chains, the layout sums, and the planted errors."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from tests import bcn_ref as R
from tests import texture_source_ref as S

GOLDEN = Path(__file__).resolve().parent / "golden" / "texture_source_pillow.npz"
KINDS = [("bc2", S.BC2), ("bc4", S.BC4), ("bc7", S.BC7)]
CHAINS = [(20, 12, 5), (3, 5, 3), (5, 3, 255)]


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _mode(blocks):
    b0 = blocks[:, 0].astype(np.int64)
    return np.where(b0 == 0, 8, np.log2(np.maximum(b0 & -b0, 1)).astype(np.int64))


def test_the_fixture_holds_what_the_rule_needs(golden):
    assert str(golden["pillow_version"]).startswith("12.")
    b = golden["bc7_blocks"]
    modes = _mode(b)
    assert [int((modes[:1024] == m).sum()) for m in range(8)] == [128] * 8  # the random blocks, the mode bits forced
    assert (modes == 8).sum() == 4 and (modes[-4:] == 8).all()  # exactly four reserved-mode blocks
    structured = b[1024:]
    sm = modes[1024:]
    for m, bits in ((0, 4), (1, 6), (2, 6), (3, 6), (7, 6)):  # every partition of every partitioned mode
        part = (structured[sm == m].astype(np.int64) @ (1 << (8 * np.arange(16, dtype=object))))
        assert {int((int(v) >> (m + 1)) & ((1 << bits) - 1)) for v in part} == set(range(1 << bits)), m
    four = [(int(x) >> 5) & 7 for x in structured[sm == 4][:, 0]]  # rotation (2 bits) and index selection behind the 5 mode bits
    assert set(four) == set(range(8))
    assert {int(x) >> 6 for x in structured[sm == 5][:, 0]} == {0, 1, 2, 3}  # mode 5's rotation
    assert golden["bc2_blocks"].shape[0] >= 256 + 64 and golden["bc4_blocks"].shape[0] >= 256 + 96
    assert GOLDEN.stat().st_size <= 2 * (GOLDEN.parent / "bcn_pillow.npz").stat().st_size + 4096


@pytest.mark.parametrize("name, fmt", KINDS)
def test_restatement_equals_pillow(golden, name, fmt):
    """Byte for byte on every block but the four whose byte 0 is 0: there Pillow 12.2 returns (0, 0, 0, 255) and the rule says (0, 0, 0, 0)."""
    blocks, texels = golden[f"{name}_blocks"], golden[f"{name}_texels"]
    mine = S.decode_blocks(fmt, blocks)
    if fmt == S.BC4:
        assert texels.shape[2] == 1 and not mine[:, :, 1:3].any() and (mine[:, :, 3] == 255).all()
        mine = mine[:, :, :1]
    keep = np.ones(blocks.shape[0], bool) if fmt != S.BC7 else blocks[:, 0] != 0
    assert int((~keep).sum()) == (4 if fmt == S.BC7 else 0)
    bad = np.flatnonzero((mine[keep] != texels[keep]).any((1, 2)))
    assert bad.size == 0, f"{name}: {bad.size} blocks differ from Pillow, first {bad[:8]}"
    if fmt == S.BC7:
        assert not mine[~keep].any()  # the hand-worked answer of the reserved mode: sixteen times (0, 0, 0, 0)
        assert (texels[~keep] == np.array([0, 0, 0, 255], np.uint8)).all()  # (what Pillow 12.2 was seen to give)


def test_srgb_forms_share_their_twins_code_words(golden):
    assert np.array_equal(S.decode_blocks(S.BC2_SRGB, golden["bc2_blocks"]), S.decode_blocks(S.BC2, golden["bc2_blocks"]))
    assert np.array_equal(S.decode_blocks(S.BC7_SRGB, golden["bc7_blocks"]), S.decode_blocks(S.BC7, golden["bc7_blocks"]))
    assert [S.is_srgb(f) for f in S.FORMATS] == [False, True, False, True, False, False, True, False, False, True]
    assert [S.block_bytes(f) for f in S.FORMATS] == [8, 8, 16, 16, 16, 16, 16, 8, 16, 16]


def _one(block):
    return S.decode_blocks(S.BC7, block[None])[0].tolist()


def test_hand_worked_bc7_blocks():
    """One block of each mode, in round numbers; interpolated entries are ((64 - w) e0 + w e1 + 32) >> 6 worked by hand."""
    # mode 6: 7 bits + p-bit 1: 0 -> 1, 127 -> 255; index 15 is weight 64, index 8 weight 34: (30 * 1 + 34 * 255 + 32) >> 6 = 136
    t = _one(S.bc7_block(6, endpoints=[(0, 0, 0, 0), (127, 127, 127, 127)], pbits=[1, 1], indices=[0, 15, 8] + [15] * 13))
    assert t[0] == [1, 1, 1, 1] and t[1] == [255] * 4 and t[2] == [136] * 4 and t[15] == [255] * 4
    # mode 5: 7-bit colour 127 -> 255, 64 -> 129; 8-bit alpha 0 and 255 under 2-bit indices: 1 is weight 21, (21 * 255 + 32) >> 6 = 84
    ends = [(127, 0, 64, 0), (127, 0, 64, 255)]
    t = _one(S.bc7_block(5, endpoints=ends, indices=[0] * 16, indices2=[1, 3] + [0] * 14))
    assert t[0] == [255, 0, 129, 84] and t[1] == [255, 0, 129, 255] and t[2] == [255, 0, 129, 0]
    t = _one(S.bc7_block(5, rotation=1, endpoints=ends, indices=[0] * 16, indices2=[1, 3] + [0] * 14))  # A and R exchanged
    assert t[0] == [84, 0, 129, 255] and t[1] == [255, 0, 129, 255] and t[2] == [0, 0, 129, 255]
    t = _one(S.bc7_block(5, rotation=3, endpoints=ends, indices=[0] * 16, indices2=[1, 3] + [0] * 14))  # A and B exchanged
    assert t[0] == [255, 0, 84, 129]
    # mode 4: 5-bit colour 0 .. 255, 6-bit alpha 0 .. 255; 2-bit index 1 -> 84, 3 -> 255; 3-bit index 3 is weight 27: (27 * 255 + 32) >> 6 = 108, index 4 weight 37: 147
    ends = [(0, 0, 0, 0), (31, 31, 31, 63)]
    t = _one(S.bc7_block(4, endpoints=ends, indices=[1, 3] + [0] * 14, indices2=[3, 4, 7] + [0] * 13))
    assert t[0] == [84, 84, 84, 108] and t[1] == [255, 255, 255, 147] and t[2] == [0, 0, 0, 255]
    t = _one(S.bc7_block(4, index_selection=1, endpoints=ends, indices=[1, 3] + [0] * 14, indices2=[3, 4, 7] + [0] * 13))  # the weights exchanged
    assert t[0] == [108, 108, 108, 84] and t[1] == [147, 147, 147, 255] and t[2] == [255, 255, 255, 0]
    # mode 0, partition 0 (texels 0, 1: subset 0; 2, 3: subset 1; 15: subset 2, and its anchor): 4 bits + p-bit, 15|1 -> 255, 0|1 -> 8, 15|0 -> 247
    t = _one(S.bc7_block(0, 0, endpoints=[(15, 0, 0)] * 2 + [(0, 15, 0)] * 2 + [(0, 0, 15), (0, 0, 0)], pbits=[1, 1, 0, 0, 1, 0], indices=[0] * 15 + [3]))
    assert t[0] == [255, 8, 8, 255] and t[2] == [0, 247, 0, 255] and t[3] == [0, 247, 0, 255]
    assert t[15] == [5, 5, 147, 255]  # weight 27 of the 3-bit table: (37 * 8 + 32) >> 6 = 5, (37 * 255 + 32) >> 6 = 147
    # mode 1, partition 13 (texels 8..15: subset 1, anchor 15): 6 bits + the subset's p-bit; 63|1 -> 255, 32|0 -> 129; index 4: (27 * 0 + 37 * 129 + 32) >> 6 = 75
    t = _one(S.bc7_block(1, 13, endpoints=[(63, 63, 63)] * 2 + [(0, 0, 0), (32, 32, 32)], pbits=[1, 0], indices=[0] * 8 + [7, 4] + [0] * 6))
    assert t[0] == [255, 255, 255, 255] and t[7] == [255] * 4 and t[8] == [129, 129, 129, 255] and t[9] == [75, 75, 75, 255] and t[10] == [0, 0, 0, 255]
    # mode 2, partition 0: 5 bits, no p-bit; 16 -> 132; subset 1 from (255, 0, 0) to (0, 255, 0) under index 1: (43 * 255 + 32) >> 6 = 171 and 84
    t = _one(S.bc7_block(2, 0, endpoints=[(16, 16, 16)] * 2 + [(31, 0, 0), (0, 31, 0)] + [(0, 0, 0)] * 2, indices=[0, 0, 1] + [0] * 13))
    assert t[0] == [132, 132, 132, 255] and t[2] == [171, 84, 0, 255] and t[3] == [255, 0, 0, 255] and t[15] == [0, 0, 0, 255]
    # mode 3, partition 0 (texels 2, 3 of every row: subset 1): 7 bits + p-bit are the 8 bits themselves
    t = _one(S.bc7_block(3, 0, endpoints=[(100, 50, 25)] * 2 + [(0, 0, 0)] * 2, pbits=[0, 1, 0, 0], indices=[0, 3] + [0] * 14))
    assert t[0] == [200, 100, 50, 255] and t[1] == [201, 101, 51, 255] and t[2] == [0, 0, 0, 255]
    # mode 7, partition 0: 5 bits + p-bit, alpha too: 31|1 -> 255, 0|0 -> 0; index 2 is weight 43: (21 * 255 + 32) >> 6 = 84
    t = _one(S.bc7_block(7, 0, endpoints=[(31, 31, 31, 31), (0, 0, 0, 0)] + [(0, 0, 0, 0)] * 2, pbits=[1, 0, 0, 0], indices=[0, 2] + [0] * 14))
    assert t[0] == [255] * 4 and t[1] == [84] * 4 and t[2] == [0] * 4
    # the reserved mode
    assert not S.decode_blocks(S.BC7, np.array([[0] + [255] * 15], np.uint8)).any()


def test_hand_worked_bc2_and_bc4_blocks():
    # BC2: alphas 0..15 in texel order, A = 17 a; the colour block is four-colour though c0 <= c1: index 3 is (P0 + 2 P1) / 3, not transparent
    alpha = int(sum(n << (4 * n) for n in range(16))).to_bytes(8, "little")
    colour = int(0x0000 | (0xFFFF << 16) | (0b11 << 32)).to_bytes(8, "little")
    t = S.decode_blocks(S.BC2, np.frombuffer(alpha + colour, np.uint8))[0]
    assert t[:, 3].tolist() == [17 * n for n in range(16)] and t[0, :3].tolist() == [170, 170, 170] and t[1, :3].tolist() == [0, 0, 0]
    # BC4: 3.13's alpha block in R; a0 = 255 > a1 = 0, index 2 is (6 * 255 + 0) / 7 = 218
    t = S.decode_blocks(S.BC4, np.frombuffer(int(255 | (0 << 8) | (0b010_001_000 << 16)).to_bytes(8, "little"), np.uint8))[0]
    assert t[:3].tolist() == [[255, 0, 0, 255], [0, 0, 0, 255], [218, 0, 0, 255]]


def _library_decode(fmt, blocks):
    """The blocks as one block row of a level 4 n texels wide, through ur_host_texture_decode_level -> (n, 16, 4)."""
    from unclerenderer_amd import hostmath
    n = blocks.shape[0]
    img = hostmath.texture_decode_level(fmt, blocks, 4 * n, 4)
    return img.reshape(4, n, 4, 4).transpose(1, 0, 2, 3).reshape(n, 16, 4)


@pytest.mark.parametrize("name, fmt", KINDS)
def test_library_decoder_equals_the_restatement_on_the_fixture(urlib, golden, name, fmt):
    blocks = golden[f"{name}_blocks"]
    assert np.array_equal(_library_decode(fmt, blocks), S.decode_blocks(fmt, blocks))
    for twin in {S.BC2: (S.BC2_SRGB,), S.BC7: (S.BC7_SRGB,)}.get(fmt, ()):
        assert np.array_equal(_library_decode(twin, blocks), S.decode_blocks(fmt, blocks))


@pytest.mark.parametrize("fmt", S.FORMATS)
@pytest.mark.parametrize("shape", CHAINS)
def test_library_chains_equal_the_restatement(urlib, fmt, shape):
    from unclerenderer_amd import hostmath
    w, h, mips = shape
    data = S.random_chain(fmt, w, h, mips, seed=fmt + w)
    assert hostmath.texture_chain_bytes(fmt, w, h, mips) == S.chain_bytes(fmt, w, h, mips) == data.size
    want = S.decode_chain(fmt, data, w, h, mips)
    at, texels = 0, 0
    for k, level in enumerate(want):
        wk, hk = S.level_size(w, k), S.level_size(h, k)
        assert level.shape == (hk, wk, 4)
        assert np.array_equal(hostmath.texture_decode_level(fmt, data[at:], wk, hk), level), (fmt, shape, k)
        at += R.level_blocks(w, h, k) * S.block_bytes(fmt)
        texels += wk * hk
    assert at == data.size
    assert int(urlib.ur_texture_transcode_bytes(w, h, mips)) == 4 * texels == S.rgba8_chain_bytes(w, h, mips) == S.transcode_chain(fmt, data, w, h, mips).size
    if fmt in R.FORMATS:  # 3.13's functions keep their results
        assert hostmath.bc_chain_bytes(fmt, w, h, mips) == data.size
        assert np.array_equal(hostmath.bc_decode_level(fmt, data, w, h), want[0])


def test_layout_sums(urlib):
    size = lambda *a: int(urlib.ur_texture_transcode_bytes(*a))  # noqa: E731
    assert size(20, 12, 5) == 4 * (240 + 60 + 15 + 2 + 1) and size(3, 5, 3) == 4 * (15 + 2 + 1) and size(5, 3, 255) == 4 * (15 + 2 + 253)
    assert size(65535, 1, 17) == 4 * sum(max(1, 65535 >> k) for k in range(17)) and size(65535, 65535, 1) == 4 * 65535 * 65535
    assert size(4, 4, 1) == 64 and size(1, 1, 255) == 4 * 255
    for bad in ((0, 4, 1), (4, 0, 1), (65536, 4, 1), (4, 65536, 1), (4, 4, 0), (4, 4, 256)):
        assert size(*bad) == 0, bad
    from unclerenderer_amd import hostmath
    assert hostmath.texture_chain_bytes(S.BC7, 20, 12, 5) == 25 * 16 and hostmath.texture_chain_bytes(S.BC4, 20, 12, 5) == 25 * 8
    assert hostmath.texture_chain_bytes(S.BC7, 5, 3, 255) == (2 + 254) * 16  # level 0 is two blocks wide
    for fmt in (28, 29, 79, 81, 84, 95, 96, 97, 100, 0):  # RGBA8, the typeless and SNORM forms, BC6H
        assert hostmath.texture_chain_bytes(fmt, 20, 12, 5) == 0, fmt
        with pytest.raises(ValueError):
            hostmath.texture_decode_level(fmt, np.zeros(64, np.uint8), 4, 4)
    with pytest.raises(ValueError):
        hostmath.texture_decode_level(S.BC7, np.zeros(31, np.uint8), 8, 4)
    out = np.zeros(64, np.uint8)
    assert urlib.ur_host_texture_decode_level(S.BC7, None, 4, 4, out.ctypes.data_as(C.c_void_p)) != 0
    assert urlib.ur_host_texture_decode_level(S.BC7, out.ctypes.data_as(C.c_void_p), 0, 4, out.ctypes.data_as(C.c_void_p)) != 0


def test_planted_errors_change_bytes(golden):
    """Each planted mistake changes bytes on the inputs the tests use: the fixture's blocks for the decode, the three chains for the pitch."""
    b7, b2 = golden["bc7_blocks"], golden["bc2_blocks"]
    want = S.decode_blocks(S.BC7, b7)
    modes = _mode(b7)
    for fault, seen_in in (("pbit_above", (0, 1, 3, 6, 7)), ("no_round", range(8)), ("anchor15", (0, 1, 2, 3, 7)), ("no_rotation", (4, 5)),
                           ("no_index_selection", (4,)), ("no_replication", (0, 1, 2, 4, 5, 7)), ("swap3", (0, 2))):  # (modes 3 and 6 hold 8 bits: nothing to replicate)
        changed = (S.decode_blocks(S.BC7, b7, (fault,)) != want).any((1, 2))
        assert changed.any(), fault
        assert set(modes[changed].tolist()) == set(seen_in), (fault, sorted(set(modes[changed].tolist())))
    assert not np.array_equal(S.decode_blocks(S.BC2, b2, ("bc2_shift",)), S.decode_blocks(S.BC2, b2))
    for w, h, mips in CHAINS:
        data = S.random_chain(S.BC7, w, h, mips, seed=7)
        assert not np.array_equal(S.transcode_chain(S.BC7, data, w, h, mips, ("pitch",)), S.transcode_chain(S.BC7, data, w, h, mips)), (w, h, mips)
