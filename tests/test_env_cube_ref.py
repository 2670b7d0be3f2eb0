"""The environment cube build without a GPU (include/ur_env_cube.h): hand-worked answers, ur_host_env_cube_build byte-equal
to the numpy restatement (tests/env_cube_ref.py) over random payloads that reach all 14 BC6H modes and the reserved ones, the shipped cube
through the host build against the staging ur_stage_env_cube runs, and planted errors in the restatement that must each change bytes."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from tests import env_cube_ref as R

ASSETS = Path(__file__).parent / "golden" / "assets"
EDGES = (1, 2, 3, 4, 5, 6, 7, 8, 12, 16, 33)
FORMATS = (R.RGBA16F, R.UF16, R.SF16)


def cases():
    """(format, base, mips): every edge as a full chain and as one level, in every format."""
    return [(fmt, base, mips) for fmt in FORMATS for base in EDGES for mips in sorted({1, R.full_chain(base)})]


def host(payload, fmt, base, mips):
    from unclerenderer_amd import hostmath
    return hostmath.env_cube_build(payload, fmt, base, mips)


def test_source_bytes_by_hand(urlib):
    # BC6H, base 4, 3 mips: levels of edge 4, 2, 1 are one block each: 3 blocks * 16 bytes * 6 faces
    assert urlib.ur_env_cube_source_bytes(R.UF16, 4, 3) == 288 and urlib.ur_env_cube_source_bytes(R.SF16, 4, 3) == 288
    # RGBA16F: (16 + 4 + 1) texels * 8 bytes * 6 faces
    assert urlib.ur_env_cube_source_bytes(R.RGBA16F, 4, 3) == 1008
    assert urlib.ur_env_cube_source_bytes(R.SF16, 256, 9) == 6 * 16 * (64 * 64 + 32 * 32 + 16 * 16 + 8 * 8 + 4 * 4 + 2 * 2 + 1 + 1 + 1)
    assert urlib.ur_env_cube_source_bytes(R.SF16, 5, 1) == 6 * 4 * 16  # a 5 x 5 level is 2 x 2 blocks
    for fmt, base, mips in ((R.SF16, 0, 1), (R.SF16, 4, 0), (R.SF16, 4, 17), (97, 4, 3), (0, 4, 3), (71, 4, 3)):
        assert urlib.ur_env_cube_source_bytes(fmt, base, mips) == 0
    for fmt, base, mips in cases():
        assert urlib.ur_env_cube_source_bytes(fmt, base, mips) == R.source_bytes(fmt, base, mips)


def test_edge_1_cube_by_hand(urlib):
    """Six faces of one texel: face f is the texel (f + 1, 10 f, 100 + f, 1.0). A face's ring is 8 texels. Folding an edge of a one-texel
    face lands on the neighbour's only texel; a corner clamps j into the face first, so it is the left or right neighbour's texel.
    D3D's faces: +X (1, -t, -s), -X (-1, -t, s), +Y (s, 1, t), -Y (s, -1, -t), +Z (s, -t, 1), -Z (-s, -t, -1). So for +X: left (s < 0)
    is +z = +Z, right is -Z, up (t < 0) is +y = +Y, down is -Y; and so on for each face, written out:"""
    PX, NX, PY, NY, PZ, NZ = range(6)
    #          left right up  down
    around = {PX: (PZ, NZ, PY, NY), NX: (NZ, PZ, PY, NY), PY: (NX, PX, NZ, PZ), NY: (NX, PX, PZ, NZ), PZ: (NX, PX, PY, NY), NZ: (PX, NX, PY, NY)}
    texel = lambda f: [f + 1, 10 * f, 100 + f, 0x3C00]  # noqa: E731
    payload = np.array([texel(f) for f in range(6)], np.uint16)
    got, bad = host(payload.view(np.uint8).reshape(-1), R.RGBA16F, 1, 1)
    assert bad == 0 and got.shape == (R.texels_of(1, 1), 4) == (6 * 9 + 9 * 6, 4)
    faces = got[:54].reshape(6, 3, 3, 4)
    for f, (left, right, up, down) in around.items():
        want = [[left, up, right],   # the corners take the left / right neighbour: j clamps first, then i folds
                [left, f, right],
                [left, down, right]]
        assert faces[f].tolist() == [[texel(g) for g in row] for row in want], f
    assert np.array_equal(got, R.build(urlib, payload.view(np.uint8).reshape(-1), R.RGBA16F, 1, 1)[0])


def test_edge_2_corners_by_hand(urlib):
    """Face +Z (s, -t, 1) of an edge-2 cube whose texel (face, j, i) is (face, i, j, 1.0). Its left neighbour is -X (-1, -t, s): the ring
    column i = -1 folds to -X's column s = +1/2 (i = 1) in the same row. A corner clamps j: corner (-1, -1) reads row 0, corner (-1, 2) row 1.
    Its right neighbour is +X (1, -t, -s): ring column i = 2 folds to +X's column i = 0 (s = -1/2, since z = -s = 1/2)."""
    payload = np.array([[[[f, i, j, 0x3C00] for i in range(2)] for j in range(2)] for f in range(6)], np.uint16)
    got, _ = host(payload.view(np.uint8).reshape(-1), R.RGBA16F, 2, 1)
    pz = got[:6 * 16].reshape(6, 4, 4, 4)[4]
    assert pz[0, 0].tolist() == [1, 1, 0, 0x3C00] and pz[3, 0].tolist() == [1, 1, 1, 0x3C00]  # from -X, i = 1, j = 0 and 1
    assert pz[0, 3].tolist() == [0, 0, 0, 0x3C00] and pz[3, 3].tolist() == [0, 0, 1, 0x3C00]  # from +X, i = 0, j = 0 and 1
    assert pz[1, 0].tolist() == [1, 1, 0, 0x3C00] and pz[2, 3].tolist() == [0, 0, 1, 0x3C00]  # the ring's edge texels beside them
    # up is +Y (s, 1, t): +Z's ring row j = -1 (y = 1 + 1/2 folded) lands on +Y's last row (t = z = 1/2), the same column
    assert pz[0, 1].tolist() == [2, 0, 1, 0x3C00] and pz[0, 2].tolist() == [2, 1, 1, 0x3C00]


def test_one_pair_entry_in_bytes(urlib):
    """Edge 1, one level: the pair section starts behind 54 bordered texels (432 bytes). Entry (f = 0, j = 0, i = 1) is entry 1: R G B of
    bordered texel (1, 0) of +X - the ring's top, +Y's texel - then R G B of (1, 1), +X's own texel; little-endian halves."""
    texel = lambda f: [0x0101 * (f + 1), 0x1000 + f, 0x2000 + f, 0x3C00]  # noqa: E731
    payload = np.array([texel(f) for f in range(6)], np.uint16)
    got, _ = host(payload.view(np.uint8).reshape(-1), R.RGBA16F, 1, 1)
    raw = got.view(np.uint8).reshape(-1)
    assert raw[432 + 12:432 + 24].tolist() == [0x03, 0x03, 0x02, 0x10, 0x02, 0x20, 0x01, 0x01, 0x00, 0x10, 0x00, 0x20]
    assert raw.size == 432 + 6 * 2 * 3 * 12


def test_reserved_rule_matches_the_decoder(urlib):
    """The device counts reserved blocks from a block's first byte (ur_bc6h::reserved_mode: (byte & 0x13) == 0x13); the decoder's own
    answer for every first byte is the rule."""
    out = np.zeros((16, 4), np.uint16)
    for byte0 in range(256):
        block = bytes([byte0]) + bytes(range(1, 16))
        ok = urlib.ur_bc6h_decode_block(block, 1, out.ctypes.data_as(C.c_void_p))
        assert (ok == 0) == ((byte0 & 0x13) == 0x13), byte0


@pytest.fixture(scope="module")
def built(urlib):
    """{case: (payload, the restatement's cube, its reserved count)}: computed once, shared and left unchanged."""
    out = {}
    for k, (fmt, base, mips) in enumerate(cases()):
        payload = R.random_payload(1000 + k, fmt, base, mips)
        want, bad = R.build(urlib, payload, fmt, base, mips)
        want.setflags(write=False)
        out[(fmt, base, mips)] = (payload, want, bad)
    return out


def test_random_payloads_reach_every_mode(urlib, built):
    modes, reserved = set(), 0
    ends = np.zeros(12, np.int32)
    for (fmt, base, mips), (payload, _, bad) in built.items():
        if fmt == R.RGBA16F:
            continue
        reserved += bad
        for block in payload.reshape(-1, 16):
            modes.add(urlib.ur_bc6h_block_endpoints(block.tobytes(), int(fmt == R.SF16), ends.ctypes.data_as(C.c_void_p)))
    assert modes == set(range(15)) and reserved >= 1, (sorted(modes), reserved)


@pytest.mark.parametrize("fmt", FORMATS)
def test_host_build_is_the_restatement(urlib, built, fmt):
    for (f, base, mips), (payload, want, bad) in built.items():
        if f != fmt:
            continue
        got, got_bad = host(payload, f, base, mips)
        assert got_bad == bad, (f, base, mips)
        same = got.view(np.uint8) == want.view(np.uint8)
        assert same.all(), f"format {f}, base {base}, {mips} mips: {np.count_nonzero(~same)} bytes differ, first at {int(np.flatnonzero(~same.reshape(-1))[0])}"


def test_fixture_through_the_host_build(urlib):
    """tests/golden/assets/output_pmrem.dds (256, 9 levels, BC6H_SF16): the host build of its payload is byte-equal to the staging over
    ur_dds_decode_rgba16f's texels - reached through the host entry point, since decoded texels are an RGBA16F payload as they lie."""
    from unclerenderer_amd import assets, lib
    payload, fmt, base, mips = assets.load_env_cube_dds_source(ASSETS / "output_pmrem.dds")
    assert (fmt, base, mips) == (lib.UR_ENV_SOURCE_BC6H_SF16, 256, 9) and payload.dtype == np.uint8 and payload.size == urlib.ur_env_cube_source_bytes(fmt, base, mips)
    texels, base2, mips2, bad = assets.load_env_cube_dds(ASSETS / "output_pmrem.dds")
    assert (base2, mips2) == (base, mips)
    got, got_bad = host(payload, fmt, base, mips)
    want, _ = host(texels.view(np.uint8).reshape(-1), lib.UR_ENV_SOURCE_RGBA16F, base, mips)
    assert got_bad == bad == 0 and np.array_equal(got, want)
    # the interior of mip 0's first face is the decoded face itself
    assert np.array_equal(got[:258 * 258].reshape(258, 258, 4)[1:257, 1:257], texels[:256 * 256].reshape(256, 256, 4))
    assert assets.load_env_cube_dds_source((ASSETS / "output_pmrem.dds").read_bytes())[1:] == (fmt, base, mips)


def test_source_loader_refusals():
    from unclerenderer_amd import assets
    with pytest.raises(ValueError):
        assets.load_env_cube_dds_source(ASSETS / "PreintegratedGF.dds")  # not a cube
    data = bytearray((ASSETS / "output_pmrem.dds").read_bytes())
    data[140:144] = (2).to_bytes(4, "little")  # the DX10 header's array size: two cubes
    with pytest.raises(ValueError):
        assets.load_env_cube_dds_source(bytes(data))


@pytest.mark.parametrize("fault", R.FAULTS)
def test_planted_errors_change_bytes(urlib, built, fault):
    """Each planted error in the restatement changes the bytes of a case the host build is held to: the comparison above sees it."""
    fmt, base, mips = (R.SF16, 6, 3) if fault in ("wrong_column", "mips_outer") else (R.RGBA16F, 5, 3)
    payload, want, _ = built[(fmt, base, mips)]
    wrong, _ = R.build(urlib, payload, fmt, base, mips, fault=fault)
    assert wrong.shape == want.shape and not np.array_equal(wrong, want), fault
