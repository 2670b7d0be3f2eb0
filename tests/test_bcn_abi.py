"""The BC texel formats without a GPU: the header's five constants and the struct sizes against a compiled probe, csrc/bc_host.cpp built by
the plain host compiler, the new symbols declared, exported and bound, the DDS route (ur_dds_parse_texture2d, assets.load_texture_dds) on
files built here with struct.pack, and hotpath.pack_texture_bc's length check."""
import ctypes as C
import re
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import bcn_ref as R

ROOT = Path(__file__).resolve().parent.parent
NEW = ("ur_host_bc_chain_bytes", "ur_host_bc_decode_level", "ur_dds_parse_texture2d")
FOURCC = {"DXT1": 71, "DXT5": 77, "ATI2": 83, "BC5U": 83}
ASSET_EINVAL, ASSET_EFORMAT, ASSET_EUNSUPPORTED = -1, -2, -3  # include/ur_assets.h


def _cxx():
    exe = shutil.which("g++") or shutil.which("c++")
    assert exe, "no host C++ compiler"
    return exe


def test_header_constants_and_struct_sizes_against_a_compiled_probe(tmp_path):
    from unclerenderer_amd import lib
    src = tmp_path / "probe.cpp"
    src.write_text('#include <stdio.h>\n#include "ur_raster.h"\n#include "ur_assets.h"\n#include "ur_host.h"\n'
                   'int main() { printf("%u %u %u %u %u %u %u %zu %zu %zu\\n", UR_TEXTURE_BC1_UNORM, UR_TEXTURE_BC1_UNORM_SRGB, UR_TEXTURE_BC3_UNORM, '
                   'UR_TEXTURE_BC3_UNORM_SRGB, UR_TEXTURE_BC5_UNORM, UR_TEXTURE_R8G8B8A8_UNORM, UR_TEXTURE_R8G8B8A8_UNORM_SRGB, sizeof(ur_texture2d), '
                   'sizeof(ur_material), sizeof(ur_dds_info)); return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.run([_cxx(), "-std=c++17", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [71, 72, 77, 78, 83, 28, 29, 16, 80, 36]
    assert (lib.UR_TEXTURE_BC1_UNORM, lib.UR_TEXTURE_BC1_UNORM_SRGB, lib.UR_TEXTURE_BC3_UNORM, lib.UR_TEXTURE_BC3_UNORM_SRGB, lib.UR_TEXTURE_BC5_UNORM) == (71, 72, 77, 78, 83)
    assert (R.BC1, R.BC1_SRGB, R.BC3, R.BC3_SRGB, R.BC5) == (71, 72, 77, 78, 83)
    assert C.sizeof(lib.Texture2D) == 16 and C.sizeof(lib.Material) == 80 and C.sizeof(lib.DdsInfo) == 36


def test_the_host_unit_builds_with_the_plain_compiler_and_decodes_the_same(tmp_path, urlib):
    """csrc/bc_decode.h has no HIP in it: g++ builds csrc/bc_host.cpp, and that build gives the library's bytes."""
    so = tmp_path / "libbc_host.so"
    subprocess.run([_cxx(), "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", str(ROOT / "unclerenderer_amd" / "csrc" / "bc_host.cpp"), "-o", str(so)],
                   check=True)
    plain = C.CDLL(str(so))
    plain.ur_host_bc_chain_bytes.restype = C.c_uint64
    assert plain.ur_host_bc_chain_bytes(C.c_uint32(R.BC1), C.c_uint32(20), C.c_uint32(12), C.c_uint32(5)) == 200
    for fmt in (R.BC1, R.BC3, R.BC5):
        data = R.random_chain(fmt, 64, 8, 1, seed=fmt)
        a, b = np.zeros((8, 64, 4), np.uint8), np.zeros((8, 64, 4), np.uint8)
        for f, out in ((plain.ur_host_bc_decode_level, a), (urlib.ur_host_bc_decode_level, b)):
            assert f(C.c_uint32(fmt), data.ctypes.data_as(C.c_void_p), C.c_uint32(64), C.c_uint32(8), out.ctypes.data_as(C.c_void_p)) == 0
        assert np.array_equal(a, b) and np.array_equal(a, R.decode_level(fmt, data, 64, 8))


def test_symbols_declared_exported_and_bound(urlib):
    from unclerenderer_amd import assets, hostmath, hotpath, lib
    strip = lambda text: re.sub(r"/\*.*?\*/", "", text, flags=re.S)  # noqa: E731
    host, ast = (strip((ROOT / "include" / n).read_text()) for n in ("ur_host.h", "ur_assets.h"))
    assert re.search(r"\bur_host_bc_chain_bytes\s*\(", host) and re.search(r"\bur_host_bc_decode_level\s*\(", host) and re.search(r"\bur_dds_parse_texture2d\s*\(", ast)
    for name in NEW:
        assert name in lib.SIGNATURES and getattr(urlib, name) is not None
    assert callable(hotpath.pack_texture_bc) and callable(assets.load_texture_dds) and callable(hostmath.bc_decode_level) and callable(hostmath.bc_chain_bytes)
    # no entry point was added to the hot path's header
    assert "bc" not in re.findall(r"\bur_(\w+)\s*\(", strip((ROOT / "include" / "ur_hotpath.h").read_text()))


def _dds(width, height, mips, payload, dxgi=None, fourcc=None, cube=False, array=1, volume=False):
    """A DDS file: DX10 header when `dxgi` is given, else a legacy FourCC header."""
    cc = b"DX10" if dxgi is not None else fourcc.encode()
    caps2 = (0xFE00 if cube and dxgi is None else 0) | (0x200000 if volume else 0)
    hdr = struct.pack("<4sIIIIIII44xII4sIIIIIIIII4x", b"DDS ", 124, 0x1 | 0x2 | 0x4 | 0x1000 | 0x20000, height, width, 0, 0, mips,
                      32, 0x4, cc, 0, 0, 0, 0, 0, 0x1000 | 0x400000, caps2, 0, 0)
    assert len(hdr) == 128
    if dxgi is not None:
        hdr += struct.pack("<IIIII", dxgi, 3, 0x4 if cube else 0, array, 0)
    return hdr + bytes(payload)


def _chain(fmt, w, h, mips, seed=1):
    if fmt in (28, 29):
        n = sum(max(1, w >> k) * max(1, h >> k) for k in range(mips)) * 4
        return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)
    return R.random_chain(fmt, w, h, mips, seed)


@pytest.mark.parametrize("fmt", [28, 29, 71, 72, 77, 78, 83])
def test_dds_dx10_formats(urlib, fmt):
    from unclerenderer_amd import assets
    w, h, mips = 20, 12, 5
    payload = _chain(fmt, w, h, mips)
    info = assets.parse_texture_dds(_dds(w, h, mips, payload, dxgi=fmt))
    per = (4, 1) if fmt in (28, 29) else (R.block_bytes(fmt), 4)
    assert (info.width, info.height, info.mip_count, info.slices, info.is_cube, info.dxgi_format, info.header_size, info.bytes_per_block, info.block_dim) == \
        (w, h, mips, 1, 0, fmt, 148, per[0], per[1])
    got = assets.load_texture_dds(_dds(w, h, mips, payload, dxgi=fmt) + b"trailing bytes are not the chain's")
    if fmt in (28, 29):
        levels, srgb = got
        assert srgb == (fmt == 29) and [a.shape for a in levels] == [(12, 20, 4), (6, 10, 4), (3, 5, 4), (1, 2, 4), (1, 1, 4)]
        assert np.array_equal(np.concatenate([a.reshape(-1) for a in levels]), payload)
    else:
        data, gw, gh, gm, gf = got
        assert (gw, gh, gm, gf) == (w, h, mips, fmt) and data == payload.tobytes() and len(data) == 25 * R.block_bytes(fmt)


@pytest.mark.parametrize("fourcc", sorted(FOURCC))
def test_dds_legacy_fourccs(urlib, fourcc):
    from unclerenderer_amd import assets
    fmt = FOURCC[fourcc]
    payload = _chain(fmt, 3, 5, 3)
    info = assets.parse_texture_dds(_dds(3, 5, 3, payload, fourcc=fourcc))
    assert (info.dxgi_format, info.header_size, info.width, info.height, info.mip_count, info.bytes_per_block) == (fmt, 128, 3, 5, 3, R.block_bytes(fmt))
    data, w, h, mips, got = assets.load_texture_dds(_dds(3, 5, 3, payload, fourcc=fourcc))
    assert (w, h, mips, got) == (3, 5, 3, fmt) and data == payload.tobytes()


def test_dds_refusals(urlib):
    from unclerenderer_amd import lib
    assets_h = (ROOT / "include" / "ur_assets.h").read_text()
    assert [int(re.search(r"#define %s \((-\d)\)" % n, assets_h).group(1)) for n in ("UR_ASSET_EINVAL", "UR_ASSET_EFORMAT", "UR_ASSET_EUNSUPPORTED")] == [-1, -2, -3]
    info = lib.DdsInfo()
    parse = lambda data: urlib.ur_dds_parse_texture2d(data, len(data), C.byref(info))  # noqa: E731
    good = _chain(71, 16, 16, 5)
    assert parse(_dds(16, 16, 5, good, dxgi=71)) == 0
    assert parse(_dds(16, 16, 5, good, dxgi=71, cube=True)) == ASSET_EUNSUPPORTED
    assert parse(_dds(16, 16, 5, good, fourcc="DXT1", cube=True)) == ASSET_EUNSUPPORTED
    assert parse(_dds(16, 16, 5, good, dxgi=71, array=2)) == ASSET_EUNSUPPORTED
    assert parse(_dds(16, 16, 5, good, fourcc="DXT1", volume=True)) == ASSET_EUNSUPPORTED
    assert parse(_dds(16, 16, 5, good[:-1], dxgi=71)) == ASSET_EFORMAT      # truncated by a byte
    assert parse(_dds(16, 16, 5, good[:-1], fourcc="DXT1")) == ASSET_EFORMAT
    assert parse(_dds(16, 16, 5, bytes(16 * 30), dxgi=98)) == ASSET_EUNSUPPORTED  # BC7
    for other in (74, 80, 84, 95):  # BC2, BC4, BC5_SNORM, BC6H
        assert parse(_dds(16, 16, 5, bytes(16 * 30), dxgi=other)) == ASSET_EUNSUPPORTED
    assert parse(_dds(16, 16, 5, bytes(16 * 30), fourcc="DXT3")) == ASSET_EUNSUPPORTED
    assert parse(b"DDX " + _dds(16, 16, 5, good, dxgi=71)[4:]) == ASSET_EFORMAT
    assert parse(_dds(65536, 1, 1, bytes(8 * 16384), dxgi=71)) == ASSET_EFORMAT
    assert urlib.ur_dds_parse_texture2d(None, 200, C.byref(info)) == ASSET_EINVAL
    # ur_dds_parse stays as it was: it does not take these formats
    data = _dds(16, 16, 5, good, dxgi=71)
    assert urlib.ur_dds_parse(data, len(data), C.byref(info)) == ASSET_EUNSUPPORTED


def test_load_texture_dds_applies_make_srgb_format(urlib):
    from unclerenderer_amd import assets
    for fmt, want in ((71, 72), (77, 78), (83, 83), (72, 72), (78, 78)):
        data = _dds(8, 8, 2, _chain(fmt, 8, 8, 2), dxgi=fmt)
        assert assets.load_texture_dds(data, srgb=True)[4] == want and assets.load_texture_dds(data)[4] == fmt
    for fmt in (28, 29):
        data = _dds(8, 8, 2, _chain(fmt, 8, 8, 2), dxgi=fmt)
        assert assets.load_texture_dds(data, srgb=True)[1] is True and assets.load_texture_dds(data)[1] == (fmt == 29)
    for fourcc, want in (("DXT1", 72), ("DXT5", 78), ("ATI2", 83), ("BC5U", 83)):
        fmt = FOURCC[fourcc]
        assert assets.load_texture_dds(_dds(8, 8, 2, _chain(fmt, 8, 8, 2), fourcc=fourcc), srgb=True)[4] == want


def test_load_texture_dds_from_a_path(urlib, tmp_path):
    from unclerenderer_amd import assets
    payload = _chain(77, 20, 12, 5)
    path = tmp_path / "t.dds"
    path.write_bytes(_dds(20, 12, 5, payload, dxgi=77))
    assert assets.load_texture_dds(path, srgb=True) == (payload.tobytes(), 20, 12, 5, 78)
    with pytest.raises(ValueError):
        assets.load_texture_dds(_dds(20, 12, 5, payload[:-16], dxgi=77))


def test_pack_texture_bc_checks_the_length_before_it_touches_a_device(urlib, monkeypatch):
    from unclerenderer_amd import hotpath
    monkeypatch.setattr(hotpath.tensors, "to_device", lambda *args: pytest.fail("a refused payload must not be uploaded"))
    good = R.random_chain(R.BC3, 20, 12, 5, seed=3)
    for payload in (good[:-1], np.concatenate([good, good[:16]]), good[:16], b""):
        with pytest.raises(ValueError, match="bytes"):
            hotpath.pack_texture_bc(payload, 20, 12, 5, R.BC3)
    with pytest.raises(ValueError, match="bytes"):
        hotpath.pack_texture_bc(good, 20, 12, 5, R.BC1)  # BC3's bytes are twice BC1's
    for bad in ((0, 12, 5, R.BC3), (20, 12, 0, R.BC3), (20, 12, 256, R.BC3), (20, 12, 5, 28), (20, 12, 5, 98), (65536, 12, 5, R.BC3)):
        with pytest.raises(ValueError, match="no BC chain"):
            hotpath.pack_texture_bc(good, *bad)
