"""The texture transcode without a GPU: the header's five source macros and the struct sizes against a compiled
probe, the new symbols declared, exported and bound, csrc/bc_host.cpp built by the plain host compiler, every refusal of
ur_texture_transcode that is decided before a device is needed, the DDS route of the new formats with its refusals, what keeps
refusing them (ur_dds_parse_texture2d, pack_texture_bc, the sampler's host functions), and the kernels' resources from the built
library's metadata."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

from tests import texture_source_ref as S
from tests.test_bcn_abi import ASSET_EFORMAT, ASSET_EINVAL, ASSET_EUNSUPPORTED, ROOT, _cxx, _dds

NEW = ("ur_texture_transcode_bytes", "ur_texture_transcode", "ur_host_texture_chain_bytes", "ur_host_texture_decode_level", "ur_dds_parse_texture2d_source")
FOURCC = {"DXT1": 71, "DXT3": 74, "DXT5": 77, "ATI1": 80, "BC4U": 80, "ATI2": 83, "BC5U": 83}


def test_header_macros_and_struct_sizes_against_a_compiled_probe(tmp_path):
    from unclerenderer_amd import lib
    src = tmp_path / "probe.cpp"
    src.write_text('#include <stdio.h>\n#include "ur_raster.h"\n#include "ur_assets.h"\n#include "ur_host.h"\n'
                   'int main() { printf("%u %u %u %u %u %zu %zu\\n", UR_TEXTURE_SOURCE_BC2_UNORM, UR_TEXTURE_SOURCE_BC2_UNORM_SRGB, UR_TEXTURE_SOURCE_BC4_UNORM, '
                   'UR_TEXTURE_SOURCE_BC7_UNORM, UR_TEXTURE_SOURCE_BC7_UNORM_SRGB, sizeof(ur_texture2d), sizeof(ur_dds_info)); return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.run([_cxx(), "-std=c++17", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [74, 75, 80, 98, 99, 16, 36]
    assert (lib.UR_TEXTURE_SOURCE_BC2_UNORM, lib.UR_TEXTURE_SOURCE_BC2_UNORM_SRGB, lib.UR_TEXTURE_SOURCE_BC4_UNORM, lib.UR_TEXTURE_SOURCE_BC7_UNORM,
            lib.UR_TEXTURE_SOURCE_BC7_UNORM_SRGB) == (74, 75, 80, 98, 99) == (S.BC2, S.BC2_SRGB, S.BC4, S.BC7, S.BC7_SRGB)
    raster = (ROOT / "include" / "ur_raster.h").read_text()
    for name, value in (("BC2_UNORM", 74), ("BC2_UNORM_SRGB", 75), ("BC4_UNORM", 80), ("BC7_UNORM", 98), ("BC7_UNORM_SRGB", 99)):
        assert re.search(r"#define UR_TEXTURE_SOURCE_%s \(%du\)" % (name, value), raster), name  # in parentheses: the bare list is pinned elsewhere


def test_symbols_declared_exported_and_bound(urlib):
    from unclerenderer_amd import assets, hostmath, hotpath, lib
    strip = lambda text: re.sub(r"/\*.*?\*/", "", text, flags=re.S)  # noqa: E731
    where = {"ur_texture_transcode_bytes": "ur_raster.h", "ur_texture_transcode": "ur_raster.h", "ur_host_texture_chain_bytes": "ur_host.h",
             "ur_host_texture_decode_level": "ur_host.h", "ur_dds_parse_texture2d_source": "ur_assets.h"}
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, strip((ROOT / "include" / where[name]).read_text())), name
        assert name in lib.SIGNATURES and getattr(urlib, name) is not None
    assert callable(hotpath.HotPath.transcode_texture) and callable(assets.parse_texture_dds_source) and callable(assets.load_texture_dds_source)
    assert callable(hostmath.texture_decode_level) and callable(hostmath.texture_chain_bytes)
    # nothing is wired into the frame: its header has no new entry point
    assert "transcode" not in strip((ROOT / "include" / "ur_frame.h").read_text())


def test_the_host_unit_builds_with_the_plain_compiler_and_decodes_the_same(tmp_path, urlib):
    """csrc/bc_wide_decode.h has no HIP in it: g++ -Wall -Wextra -Werror builds csrc/bc_host.cpp, and that build gives the library's bytes."""
    so = tmp_path / "libbc_host.so"
    subprocess.run([_cxx(), "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", str(ROOT / "unclerenderer_amd" / "csrc" / "bc_host.cpp"), "-o", str(so)],
                   check=True)
    plain = C.CDLL(str(so))
    plain.ur_host_texture_chain_bytes.restype = C.c_uint64
    assert plain.ur_host_texture_chain_bytes(C.c_uint32(S.BC7), C.c_uint32(20), C.c_uint32(12), C.c_uint32(5)) == 400
    for fmt in (S.BC2, S.BC4, S.BC7, 77):
        data = S.random_chain(fmt, 64, 8, 1, seed=fmt)
        a, b = np.zeros((8, 64, 4), np.uint8), np.zeros((8, 64, 4), np.uint8)
        for f, out in ((plain.ur_host_texture_decode_level, a), (urlib.ur_host_texture_decode_level, b)):
            assert f(C.c_uint32(fmt), data.ctypes.data_as(C.c_void_p), C.c_uint32(64), C.c_uint32(8), out.ctypes.data_as(C.c_void_p)) == 0
        assert np.array_equal(a, b) and np.array_equal(a, S.decode_level(fmt, data, 64, 8))


def test_transcode_refusals_that_need_no_device(urlib):
    """Every check comes before the context is looked at: a stand-in context (zero bytes, never a device's) is enough to see each refusal
    by its text, and nothing is launched. The addresses are numbers: a refused call dereferences none."""
    from unclerenderer_amd import lib
    stand_in = C.create_string_buffer(4096)
    ctx, src, dst = C.addressof(stand_in), 0x10000, 0x20000
    desc = lib.Texture2D(1, 2, 3, 4, 5, 6)

    def refused(text, *args):
        rc = urlib.ur_texture_transcode(*args, C.byref(desc))
        assert rc == lib.UR_EINVAL and text in urlib.ur_last_error().decode(), (text, rc, urlib.ur_last_error())

    refused("null", None, S.BC7, src, 8, 8, 1, dst)
    refused("null", ctx, S.BC7, None, 8, 8, 1, dst)
    refused("null", ctx, S.BC7, src, 8, 8, 1, None)
    for fmt in (28, 29, 70, 73, 76, 79, 81, 82, 84, 95, 96, 97, 100, 0):
        refused("source format", ctx, fmt, src, 8, 8, 1, dst)
    for fmt in (S.BC2, S.BC2_SRGB, 77, 78, 83, S.BC7, S.BC7_SRGB):  # 16-byte blocks
        refused("aligned to the block size", ctx, fmt, src + 8, 8, 8, 1, dst)
    for fmt in (71, 72, S.BC4):  # 8-byte blocks
        refused("aligned to the block size", ctx, fmt, src + 4, 8, 8, 1, dst)
    for off in (1, 2, 3):
        refused("4-byte aligned", ctx, S.BC7, src, 8, 8, 1, dst + off)
    for shape in ((0, 8, 1), (8, 0, 1), (65536, 8, 1), (8, 65536, 1), (8, 8, 0), (8, 8, 256)):
        refused("no chain", ctx, S.BC7, src, *shape, dst)
    # 8 x 8, one level: 64 source bytes (BC7), 256 destination bytes
    refused("overlap", ctx, S.BC7, src, 8, 8, 1, src)
    refused("overlap", ctx, S.BC7, src, 8, 8, 1, src + 60)
    refused("overlap", ctx, S.BC7, src + 240, 8, 8, 1, src)
    assert bytes(desc) == bytes(lib.Texture2D(1, 2, 3, 4, 5, 6))  # a refused call leaves the descriptor alone
    assert urlib.ur_texture_transcode(None, S.BC7, src, 8, 8, 1, dst, None) == lib.UR_EINVAL


def _chain(fmt, w, h, mips):
    return S.random_chain(fmt, w, h, mips, seed=fmt)


@pytest.mark.parametrize("fmt", S.FORMATS)
def test_dds_source_dx10_formats(urlib, fmt):
    from unclerenderer_amd import assets
    w, h, mips = 20, 12, 5
    payload = _chain(fmt, w, h, mips)
    info = assets.parse_texture_dds_source(_dds(w, h, mips, payload, dxgi=fmt))
    assert (info.width, info.height, info.mip_count, info.slices, info.is_cube, info.dxgi_format, info.header_size, info.bytes_per_block, info.block_dim) == \
        (w, h, mips, 1, 0, fmt, 148, S.block_bytes(fmt), 4)
    got = assets.load_texture_dds_source(_dds(w, h, mips, payload, dxgi=fmt) + b"trailing bytes are not the chain's")
    assert got == (payload.tobytes(), w, h, mips, fmt) and len(got[0]) == 25 * S.block_bytes(fmt)
    want = {71: 72, 74: 75, 77: 78, 98: 99}.get(fmt, fmt)  # MakeSRGBFormat
    assert assets.load_texture_dds_source(_dds(w, h, mips, payload, dxgi=fmt), srgb=True)[4] == want


@pytest.mark.parametrize("fourcc", sorted(FOURCC))
def test_dds_source_legacy_fourccs(urlib, fourcc):
    from unclerenderer_amd import assets
    fmt = FOURCC[fourcc]
    payload = _chain(fmt, 3, 5, 3)
    info = assets.parse_texture_dds_source(_dds(3, 5, 3, payload, fourcc=fourcc))
    assert (info.dxgi_format, info.header_size, info.width, info.height, info.mip_count, info.bytes_per_block) == (fmt, 128, 3, 5, 3, S.block_bytes(fmt))
    assert assets.load_texture_dds_source(_dds(3, 5, 3, payload, fourcc=fourcc)) == (payload.tobytes(), 3, 5, 3, fmt)


def test_dds_source_refusals(urlib):
    from unclerenderer_amd import assets, lib
    info = lib.DdsInfo()
    parse = lambda data: urlib.ur_dds_parse_texture2d_source(data, len(data), C.byref(info))  # noqa: E731
    good = _chain(S.BC7, 16, 16, 5)
    assert parse(_dds(16, 16, 5, good, dxgi=98)) == 0
    assert parse(_dds(16, 16, 5, good, dxgi=98, cube=True)) == ASSET_EUNSUPPORTED
    assert parse(_dds(16, 16, 5, good, dxgi=98, array=2)) == ASSET_EUNSUPPORTED
    assert parse(_dds(16, 16, 5, good, fourcc="DXT3", volume=True)) == ASSET_EUNSUPPORTED
    assert parse(_dds(16, 16, 5, good, fourcc="DXT3", cube=True)) == ASSET_EUNSUPPORTED
    assert parse(_dds(16, 16, 5, good[:-1], dxgi=98)) == ASSET_EFORMAT  # truncated by a byte
    assert parse(_dds(16, 16, 5, good[:-1], fourcc="DXT3")) == ASSET_EFORMAT
    assert parse(_dds(16, 16, 5, good[:len(good) // 2], fourcc="ATI1")) == 0 and info.bytes_per_block == 8  # BC4's chain is half as long
    for other in (70, 73, 76, 79, 81, 82, 84, 85, 94, 95, 96, 97, 100):  # typeless, BC4_SNORM, BC5_SNORM, BC6H
        assert parse(_dds(16, 16, 5, good, dxgi=other)) == ASSET_EUNSUPPORTED, other
    for fourcc in ("BC4S", "BC5S", "DXT2", "DXT4"):
        assert parse(_dds(16, 16, 5, good, fourcc=fourcc)) == ASSET_EUNSUPPORTED, fourcc
    assert parse(_dds(65536, 1, 1, bytes(16 * 16384), dxgi=98)) == ASSET_EFORMAT
    assert urlib.ur_dds_parse_texture2d_source(None, 200, C.byref(info)) == ASSET_EINVAL
    rgba = np.zeros(4 * (256 + 64 + 16 + 4 + 1), np.uint8)
    assert parse(_dds(16, 16, 5, rgba, dxgi=28)) == 0  # everything ur_dds_parse_texture2d accepts ...
    with pytest.raises(ValueError, match="not block-compressed"):  # ... but an RGBA8 file has nothing to transcode
        assets.load_texture_dds_source(_dds(16, 16, 5, rgba, dxgi=28))
    with pytest.raises(ValueError):
        assets.load_texture_dds_source(_dds(16, 16, 5, good[:-16], dxgi=98))


def test_what_keeps_refusing_the_new_formats(urlib, monkeypatch):
    """The sampler's side is as it was: its DDS route, its packer and csrc/bc_decode.h's host functions take their five formats alone."""
    from unclerenderer_amd import assets, hostmath, hotpath, lib
    info = lib.DdsInfo()
    good = _chain(S.BC7, 16, 16, 5)
    for fmt in (S.BC2, S.BC2_SRGB, S.BC4, S.BC7, S.BC7_SRGB):
        data = _dds(16, 16, 5, good, dxgi=fmt)
        assert urlib.ur_dds_parse_texture2d(data, len(data), C.byref(info)) == ASSET_EUNSUPPORTED, fmt
        with pytest.raises(ValueError):
            assets.load_texture_dds(data)
        assert hostmath.bc_chain_bytes(fmt, 16, 16, 5) == 0
        with pytest.raises(ValueError):
            hostmath.bc_decode_level(fmt, good, 16, 16)
    for fourcc in ("DXT3", "ATI1", "BC4U"):
        data = _dds(16, 16, 5, good, fourcc=fourcc)
        assert urlib.ur_dds_parse_texture2d(data, len(data), C.byref(info)) == ASSET_EUNSUPPORTED, fourcc
    monkeypatch.setattr(hotpath.tensors, "to_device", lambda *args: pytest.fail("a refused payload must not be uploaded"))
    for fmt in (S.BC7, S.BC2, S.BC4):
        with pytest.raises(ValueError, match="no BC chain"):
            hotpath.pack_texture_bc(good, 16, 16, 5, fmt)
    # transcode_texture checks the length before it touches a device
    class NoDevice(hotpath.HotPath):
        def __init__(self):
            self._L, self._ctx, self.device = urlib, None, 0  # (the payload path is told the context's device)
    for payload in (good[:-1], np.concatenate([good, good[:16]]), b""):
        with pytest.raises(ValueError, match="bytes"):
            NoDevice().transcode_texture(payload, 16, 16, 5, S.BC7)
    with pytest.raises(ValueError, match="no source chain"):
        NoDevice().transcode_texture(good, 16, 16, 5, 28)


def test_transcode_kernels_use_no_scratch_and_spill_nothing(urlib, tmp_path):
    from tests.code_objects import library_kernels
    kernels = {k: v for k, v in library_kernels(tmp_path).items() if "texture_transcode_kernel" in k}
    assert len(kernels) == 6, sorted(kernels)  # BC1, BC2, BC3, BC4, BC5, BC7
    for name, meta in kernels.items():
        assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0 and meta["sgpr_spill_count"] == 0, (name, meta)
        assert meta["vgpr_count"] <= 64, (name, meta)  # eight waves a SIMD: nothing here needs more
