"""Asset loading. IBL: DDS (BC6H cube, RG16 LUT) -> host arrays ready for HotPath.stage_env_cube / make_tables. Material textures: DDS
(RGBA8, BC1, BC3, BC5) -> what hotpath.pack_texture / pack_texture_bc take; BC blocks stay compressed, the sampler decodes them.
BC2, BC4 and BC7 too (load_texture_dds_source) -> what HotPath.transcode_texture takes: decoded to RGBA8 once, on the device.
All parsing and decoding happens in libur_hotpath.so (csrc/dds.cpp); this module only reads the file and marshals."""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np

from . import lib as _lib


def parse_dds(data: bytes) -> _lib.DdsInfo:
    info = _lib.DdsInfo()
    rc = _lib.load().ur_dds_parse(data, len(data), C.byref(info))
    if rc != 0:
        raise ValueError(f"ur_dds_parse failed ({rc})")
    return info


def load_env_cube_dds(path) -> tuple[np.ndarray, int, int, int]:
    """Returns (texels (n,4) uint16 in DDS order, base size, mip count, reserved-block count)."""
    data = Path(path).read_bytes()
    info = parse_dds(data)
    if not info.is_cube or info.slices != 6 or info.width != info.height:
        raise ValueError("not a single cube map")
    n = int(_lib.load().ur_dds_texel_count(C.byref(info)))
    out = np.zeros((n, 4), np.uint16)
    bad = C.c_uint32(0)
    rc = _lib.load().ur_dds_decode_rgba16f(data, len(data), C.byref(info), out.ctypes.data_as(C.c_void_p), C.byref(bad))
    if rc != 0:
        raise ValueError(f"ur_dds_decode_rgba16f failed ({rc})")
    return out, int(info.width), int(info.mip_count), int(bad.value)


def load_brdf_lut_dds(path) -> np.ndarray:
    """Returns (h, w, 2) uint16 R16G16_UNORM."""
    data = Path(path).read_bytes()
    info = parse_dds(data)
    out = np.zeros((info.height, info.width, 2), np.uint16)
    rc = _lib.load().ur_dds_copy_rg16(data, len(data), C.byref(info), out.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise ValueError(f"ur_dds_copy_rg16 failed ({rc})")
    return out


# MakeSRGBFormat (Source/Render/TextureLoader.cpp) for the formats the sampler takes; BC5 has no sRGB form
_SRGB_FORM = {_lib.UR_TEXTURE_R8G8B8A8_UNORM: _lib.UR_TEXTURE_R8G8B8A8_UNORM_SRGB, _lib.UR_TEXTURE_BC1_UNORM: _lib.UR_TEXTURE_BC1_UNORM_SRGB,
              _lib.UR_TEXTURE_BC3_UNORM: _lib.UR_TEXTURE_BC3_UNORM_SRGB}


def parse_texture_dds(data: bytes) -> _lib.DdsInfo:
    info = _lib.DdsInfo()
    rc = _lib.load().ur_dds_parse_texture2d(data, len(data), C.byref(info))
    if rc != 0:
        raise ValueError(f"ur_dds_parse_texture2d failed ({rc}): not a 2D DDS of RGBA8, BC1, BC3 or BC5 with its whole mip chain")
    return info


# ... and for the formats that only the transcode takes; BC4 has no sRGB form
_SRGB_SOURCE_FORM = {**_SRGB_FORM, _lib.UR_TEXTURE_SOURCE_BC2_UNORM: _lib.UR_TEXTURE_SOURCE_BC2_UNORM_SRGB,
                     _lib.UR_TEXTURE_SOURCE_BC7_UNORM: _lib.UR_TEXTURE_SOURCE_BC7_UNORM_SRGB}


def parse_texture_dds_source(data: bytes) -> _lib.DdsInfo:
    info = _lib.DdsInfo()
    rc = _lib.load().ur_dds_parse_texture2d_source(data, len(data), C.byref(info))
    if rc != 0:
        raise ValueError(f"ur_dds_parse_texture2d_source failed ({rc}): not a 2D DDS of RGBA8, BC1, BC2, BC3, BC4, BC5 or BC7 with its whole mip chain")
    return info


def load_texture_dds_source(path_or_bytes, srgb: bool = False):
    """A block-compressed source of HotPath.transcode_texture from a DDS file (a path, or the file's bytes): BC1, BC2, BC3, BC4_UNORM, BC5_UNORM
    or BC7. `srgb` applies the reference's MakeSRGBFormat: 71 -> 72, 74 -> 75, 77 -> 78, 98 -> 99. Returns (payload bytes, width, height,
    mips, format): transcode_texture's arguments. An RGBA8 file has nothing to transcode: ValueError (load_texture_dds takes it)."""
    data = bytes(path_or_bytes) if isinstance(path_or_bytes, (bytes, bytearray, memoryview)) else Path(path_or_bytes).read_bytes()
    info = parse_texture_dds_source(data)
    if info.block_dim != 4:
        raise ValueError(f"format {int(info.dxgi_format)} is not block-compressed: load_texture_dds takes it")
    fmt = int(info.dxgi_format)
    if srgb:
        fmt = _SRGB_SOURCE_FORM.get(fmt, fmt)
    w, h, mips = int(info.width), int(info.height), int(info.mip_count)
    size = sum(((max(1, w >> min(k, 16)) + 3) >> 2) * ((max(1, h >> min(k, 16)) + 3) >> 2) for k in range(mips)) * int(info.bytes_per_block)
    return data[info.header_size:info.header_size + size], w, h, mips, fmt


def load_texture_dds(path_or_bytes, srgb: bool = False):
    """A material texture from a DDS file (a path, or the file's bytes). `srgb` applies the reference's MakeSRGBFormat: 28 -> 29, 71 -> 72,
    77 -> 78, every other format as it is. Returns the arguments of the packer that takes it:
      a BC format: (payload bytes, width, height, mips, format) for hotpath.pack_texture_bc(*...);
      RGBA8:       (levels, srgb) for hotpath.pack_texture(*...), levels a list of (h, w, 4) uint8 arrays."""
    data = bytes(path_or_bytes) if isinstance(path_or_bytes, (bytes, bytearray, memoryview)) else Path(path_or_bytes).read_bytes()
    info = parse_texture_dds(data)
    fmt = int(info.dxgi_format)
    if srgb:
        fmt = _SRGB_FORM.get(fmt, fmt)
    w, h, mips = int(info.width), int(info.height), int(info.mip_count)
    sizes = [(max(1, w >> min(k, 16)), max(1, h >> min(k, 16))) for k in range(mips)]
    if info.block_dim == 4:
        size = sum(((wk + 3) >> 2) * ((hk + 3) >> 2) for wk, hk in sizes) * int(info.bytes_per_block)
        return data[info.header_size:info.header_size + size], w, h, mips, fmt
    levels, at = [], int(info.header_size)
    for wk, hk in sizes:
        levels.append(np.frombuffer(data, np.uint8, wk * hk * 4, at).reshape(hk, wk, 4).copy())
        at += wk * hk * 4
    return levels, fmt == _lib.UR_TEXTURE_R8G8B8A8_UNORM_SRGB
