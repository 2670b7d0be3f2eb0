"""DESIGN.md section 3.13 without a GPU: the numpy restatement of the BC1 / BC3 / BC5 rule (tests/bcn_ref.py) equals Pillow's decoder on the
fixture's blocks and the hand-worked entries; the library's decoder (csrc/bc_decode.h, the very functions the kernels run, through
ur_host_bc_decode_level) equals the restatement on every pair of endpoints under every index - which proves the multiply-and-shift
divisions by 3, 5 and 7 -; the layout arithmetic equals sums written out; and each planted mistake changes bytes on these inputs."""
from pathlib import Path

import numpy as np
import pytest

from tests import bcn_ref as R

GOLDEN = Path(__file__).resolve().parent / "golden" / "bcn_pillow.npz"
RAMP2 = int(sum((n & 3) << (2 * n) for n in range(16)))
RAMP3 = int(sum((n & 7) << (3 * n) for n in range(16)))


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _colour(c0, c1, idx=RAMP2):
    return np.frombuffer(int(c0 | (c1 << 16) | (idx << 32)).to_bytes(8, "little"), np.uint8)


def _alpha(a0, a1, idx=RAMP3):
    return np.frombuffer(int(a0 | (a1 << 8) | (idx << 16)).to_bytes(8, "little"), np.uint8)


@pytest.mark.parametrize("name, fmt", [("bc1", R.BC1), ("bc3", R.BC3), ("bc5", R.BC5)])
def test_restatement_equals_pillow(golden, name, fmt):
    blocks, want = golden[f"{name}_blocks"], golden[f"{name}_texels"]
    assert blocks.shape[0] >= 1024 + len(R.structured_blocks(fmt)) and np.array_equal(blocks[1024:], R.structured_blocks(fmt))
    got = R.decode_blocks(fmt, blocks)
    if fmt == R.BC5:  # Pillow gives RGB with B = 0
        assert want.shape[2] == 3 and not want[:, :, 2].any()
        assert np.array_equal(got[:, :, :3], want) and (got[:, :, 3] == 255).all()
    else:
        assert want.shape[2] == 4 and np.array_equal(got, want)
    # the fixture holds every case the rule distinguishes
    b = blocks.astype(np.int64)
    if fmt == R.BC5:
        pairs = [(b[:, 0], b[:, 1]), (b[:, 8], b[:, 9])]
    elif fmt == R.BC3:
        pairs = [(b[:, 0], b[:, 1]), (b[:, 8] | (b[:, 9] << 8), b[:, 10] | (b[:, 11] << 8))]
    else:
        pairs = [(b[:, 0] | (b[:, 1] << 8), b[:, 2] | (b[:, 3] << 8))]
    for e0, e1 in pairs:
        assert (e0 < e1).any() and (e0 == e1).any() and (e0 > e1).any()


def test_srgb_forms_share_their_twins_code_words(golden):
    assert np.array_equal(R.decode_blocks(R.BC1_SRGB, golden["bc1_blocks"]), R.decode_blocks(R.BC1, golden["bc1_blocks"]))
    assert np.array_equal(R.decode_blocks(R.BC3_SRGB, golden["bc3_blocks"]), R.decode_blocks(R.BC3, golden["bc3_blocks"]))


def test_hand_worked_answers():
    t = R.decode_blocks(R.BC1, _colour(0xF800, 0x001F)[None])[0]
    assert t[:4].tolist() == [[255, 0, 0, 255], [0, 0, 255, 255], [170, 0, 85, 255], [85, 0, 170, 255]]
    t = R.decode_blocks(R.BC1, _colour(0x001F, 0xF800)[None])[0]
    assert t[:4].tolist() == [[0, 0, 255, 255], [255, 0, 0, 255], [127, 0, 127, 255], [0, 0, 0, 0]]
    assert R.alpha_blocks(_alpha(255, 0)[None])[0, :8].tolist() == [255, 0, 218, 182, 145, 109, 72, 36]
    assert R.alpha_blocks(_alpha(0, 255)[None])[0, :8].tolist() == [0, 255, 51, 102, 153, 204, 0, 255]
    # BC3 keeps four colours under c0 <= c1; BC5 is two alpha blocks, B = 0, A = 255
    t = R.decode_blocks(R.BC3, np.concatenate([_alpha(255, 0), _colour(0x001F, 0xF800)])[None])[0]
    assert t[2].tolist() == [85, 0, 170, 218] and t[3].tolist() == [170, 0, 85, 182]
    t = R.decode_blocks(R.BC5, np.concatenate([_alpha(255, 0), _alpha(0, 255)])[None])[0]
    assert t[2].tolist() == [218, 51, 0, 255] and t[6].tolist() == [72, 0, 0, 255] and t[7].tolist() == [36, 255, 0, 255]


def _library_decode(fmt, blocks):
    """n blocks as one level of 4n x 4 texels -> (n, 16, 4)"""
    from unclerenderer_amd import hostmath
    n = blocks.shape[0]
    img = hostmath.bc_decode_level(fmt, blocks, 4 * n, 4)
    return img.reshape(4, n, 4, 4).transpose(1, 0, 2, 3).reshape(n, 16, 4)


def _endpoint_pairs():
    """Colour blocks with every pair of 5-bit endpoints (in B, and in R) and of 6-bit endpoints (in G), each pair under c0 > c1 and under
    c0 <= c1: for B and G the order is forced by a red bit on one side, for R the pair itself decides (and both orders occur)."""
    out = []
    for b0 in range(32):
        for b1 in range(32):
            out += [_colour(0x0800 | b0, b1), _colour(b0, 0x0800 | b1), _colour(b0 << 11, b1 << 11), _colour(b0, b1)]
    for g0 in range(64):
        for g1 in range(64):
            out += [_colour(0x0800 | (g0 << 5), g1 << 5), _colour(g0 << 5, 0x0800 | (g1 << 5)), _colour(g0 << 5, g1 << 5)]
    return np.stack(out)


def test_library_decoder_equals_the_rule_on_every_colour_endpoint_pair(urlib):
    colours = _endpoint_pairs()
    c0 = colours[:, 0].astype(int) | (colours[:, 1].astype(int) << 8)
    c1 = colours[:, 2].astype(int) | (colours[:, 3].astype(int) << 8)
    assert (c0 > c1).sum() > 5000 and (c0 <= c1).sum() > 5000
    assert np.array_equal(_library_decode(R.BC1, colours), R.decode_blocks(R.BC1, colours))
    bc3 = np.concatenate([np.tile(_alpha(9, 200), (colours.shape[0], 1)), colours], 1)  # BC3's forced four-colour mode over the same pairs
    assert np.array_equal(_library_decode(R.BC3, bc3), R.decode_blocks(R.BC3, bc3))
    assert np.array_equal(_library_decode(R.BC3_SRGB, bc3), R.decode_blocks(R.BC3, bc3))


def test_library_decoder_equals_the_rule_on_every_alpha_endpoint_pair(urlib):
    a0, a1 = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    head = np.stack([a0.reshape(-1), a1.reshape(-1)], 1).astype(np.uint8)
    alphas = np.concatenate([head, np.tile(_alpha(0, 0)[2:], (65536, 1))], 1)  # all eight indices in texels 0..7 (and again in 8..15)
    want = R.alpha_blocks(alphas)
    bc3 = np.concatenate([alphas, np.tile(_colour(0x1234, 0xABCD), (65536, 1))], 1)
    assert np.array_equal(_library_decode(R.BC3, bc3)[:, :, 3], want)
    bc5 = np.concatenate([alphas, alphas[::-1]], 1)
    got = _library_decode(R.BC5, bc5)
    assert np.array_equal(got[:, :, 0], want) and np.array_equal(got[:, :, 1], want[::-1]) and not got[:, :, 2].any() and (got[:, :, 3] == 255).all()


@pytest.mark.parametrize("name, fmt", [("bc1", R.BC1), ("bc3", R.BC3), ("bc5", R.BC5)])
def test_library_decoder_equals_pillow(urlib, golden, name, fmt):
    got, want = _library_decode(fmt, golden[f"{name}_blocks"]), golden[f"{name}_texels"]
    assert np.array_equal(got[:, :, :want.shape[2]], want)


def test_layout():
    from unclerenderer_amd import hostmath
    assert [R.level_blocks(20, 12, k) for k in range(5)] == [15, 6, 2, 1, 1]
    assert R.chain_bytes(R.BC1, 20, 12, 5) == 25 * 8 and R.chain_bytes(R.BC3, 20, 12, 5) == 25 * 16 == R.chain_bytes(R.BC5, 20, 12, 5)
    wide = sum((max(1, 65535 >> k) + 3) >> 2 for k in range(16)) + 1  # 65535 x 1: sixteen shrinking rows of blocks, then level 16 = one block
    assert wide == 16384 + 8192 + 4096 + 2048 + 1024 + 512 + 256 + 128 + 64 + 32 + 16 + 8 + 4 + 2 + 1 + 1 + 1
    assert R.chain_bytes(R.BC1, 65535, 1, 17) == wide * 8 == R.chain_bytes(R.BC1, 1, 65535, 17)
    assert [R.level_blocks(3, 5, k) for k in range(3)] == [2, 1, 1]
    assert R.chain_bytes(R.BC3, 1, 1, 33) == 33 * 16 and R.chain_bytes(R.BC1, 1, 1, 255) == 255 * 8
    assert R.level_offset_bytes(R.BC5, 1000, 600, 2) == (250 * 150 + 125 * 75) * 16
    for fmt in R.FORMATS:
        for w, h, mips in ((20, 12, 5), (65535, 1, 17), (1, 65535, 17), (3, 5, 3), (1, 1, 33), (1, 1, 255), (1000, 600, 3), (64, 64, 7), (65535, 65535, 255)):
            assert hostmath.bc_chain_bytes(fmt, w, h, mips) == R.chain_bytes(fmt, w, h, mips), (fmt, w, h, mips)
    for bad in ((28, 4, 4, 1), (R.BC1, 0, 4, 1), (R.BC1, 4, 0, 1), (R.BC1, 65536, 4, 1), (R.BC1, 4, 4, 0), (R.BC1, 4, 4, 256), (98, 4, 4, 1)):
        assert hostmath.bc_chain_bytes(*bad) == 0, bad


@pytest.mark.parametrize("fmt", R.FORMATS)
@pytest.mark.parametrize("shape", [(20, 12, 5), (3, 5, 3), (1, 1, 4), (37, 9, 6)])
def test_library_levels_equal_the_rule(urlib, fmt, shape):
    """Levels with edge blocks: texel (x, y) comes from block (x >> 2, y >> 2) of a ((wk + 3) >> 2)-block row, padding texels never."""
    from unclerenderer_amd import hostmath
    w, h, mips = shape
    data = R.random_chain(fmt, w, h, mips, seed=fmt * 131 + w)
    for k, level in enumerate(R.decode_chain(fmt, data, w, h, mips)):
        at = R.level_offset_bytes(fmt, w, h, k)
        assert np.array_equal(hostmath.bc_decode_level(fmt, data[at:], R.level_size(w, k), R.level_size(h, k)), level), k


def test_planted_errors_change_bytes(golden):
    """Each mistake, planted in a copy of the restatement, changes bytes on the inputs the tests use: the inputs can see it."""
    bc1, bc3 = golden["bc1_blocks"], golden["bc3_blocks"]
    assert not np.array_equal(R.decode_blocks(R.BC1, bc1, faults=("weights",)), R.decode_blocks(R.BC1, bc1))
    assert not np.array_equal(R.decode_blocks(R.BC1, bc1, faults=("no3",)), R.decode_blocks(R.BC1, bc1))
    assert not np.array_equal(R.decode_blocks(R.BC3, bc3, faults=("bc3mode",)), R.decode_blocks(R.BC3, bc3))
    assert not np.array_equal(R.decode_blocks(R.BC3, bc3, faults=("bigendian",)), R.decode_blocks(R.BC3, bc3))
    assert not np.array_equal(R.decode_blocks(R.BC5, golden["bc5_blocks"], faults=("bigendian",)), R.decode_blocks(R.BC5, golden["bc5_blocks"]))
    # the structured blocks alone see the decode faults too (they do not lean on luck in the random ones)
    for fmt, fault in ((R.BC1, "weights"), (R.BC1, "no3"), (R.BC3, "bc3mode"), (R.BC3, "bigendian"), (R.BC5, "bigendian")):
        s = R.structured_blocks(fmt)
        assert not np.array_equal(R.decode_blocks(fmt, s, faults=(fault,)), R.decode_blocks(fmt, s)), (fmt, fault)
    for fmt in (R.BC1, R.BC3, R.BC5):
        data = R.random_chain(fmt, 20, 12, 5, seed=7)
        good = R.decode_chain(fmt, data, 20, 12, 5)
        pitch = R.decode_chain(fmt, data, 20, 12, 5, faults=("pitch",))
        texels = R.decode_chain(fmt, data, 20, 12, 5, faults=("texels",))
        assert any(not np.array_equal(a, b) for a, b in zip(good, pitch)) and np.array_equal(good[0], pitch[0])  # (20 >> 2 is 5 either way; 10 >> 2 is not 3)
        assert any(not np.array_equal(a, b) for a, b in zip(good, texels)) and np.array_equal(good[0], texels[0])
        data = R.random_chain(fmt, 3, 5, 3, seed=8)
        assert any(not np.array_equal(a, b) for a, b in zip(R.decode_chain(fmt, data, 3, 5, 3), R.decode_chain(fmt, data, 3, 5, 3, faults=("texels",))))


def test_decode_level_refuses_what_it_cannot_describe(urlib):
    import ctypes as C
    from unclerenderer_amd import hostmath, lib
    blocks, out = (C.c_uint8 * 16)(), (C.c_uint8 * 64)()
    f = urlib.ur_host_bc_decode_level
    assert f(R.BC3, blocks, 4, 4, out) == 0
    assert f(R.BC3, None, 4, 4, out) == lib.UR_EINVAL and f(R.BC3, blocks, 4, 4, None) == lib.UR_EINVAL
    assert f(28, blocks, 4, 4, out) == lib.UR_EINVAL and f(98, blocks, 4, 4, out) == lib.UR_EINVAL  # RGBA8, BC7
    assert f(R.BC3, blocks, 0, 4, out) == lib.UR_EINVAL and f(R.BC3, blocks, 4, 0, out) == lib.UR_EINVAL
    with pytest.raises(ValueError):
        hostmath.bc_decode_level(R.BC1, bytes(8), 5, 4)  # two blocks across, one given
