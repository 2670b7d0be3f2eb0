"""An environment from a lat-long Radiance .hdr panorama, on the device: functions over a HotPath.

    rgbe = assets.load_panorama_hdr(path)                          # the file's texels, uint8 [H, W, 4]
    cube = environment.bake_panorama(hp, rgbe, W, H, base_size)    # the staged cube make_tables takes, log2(base_size) + 1 mips

panorama_to_cube is the new step (ur_env_panorama: panorama -> the cube's top level); bake_panorama chains it into
HotPath.prefilter_env_cube and HotPath.build_env_cube. Everything runs on the context's stream; nothing is synchronised or read back.

An environment with no outside asset: the project's own sky, and the BRDF LUT beside it.

    cube = environment.bake_sky(hp, fc.sky, base_size)             # lit by LightDirection / LightColor; again whenever the sun moves
    lut = environment.brdf_lut(hp)                                 # 128 x 32, in place of assets.load_brdf_lut_dds's
    tables = hp.make_tables(shadow, cube, base_size, base_size.bit_length(), lut)

sky_to_cube is ur_env_sky (sky constants -> the cube's top level), brdf_lut is ur_brdf_lut."""
from __future__ import annotations

import ctypes as C

import torch

from . import hostmath
from . import lib as _lib
from .hotpath import tensors
from .hotpath.tensors import _ptr, nbytes


def panorama_to_cube(hp, rgbe, width: int, height: int, base_size: int, taps=None, *, out=None) -> torch.Tensor:
    """ur_env_panorama: the RGBE texels of a width x height panorama (a device tensor of 4 * width * height bytes, or an array or bytes,
    uploaded here; assets.load_panorama_hdr) become the top level of an HDR cube: six RGBA16F faces of edge base_size as an int16 device
    tensor [6, base_size, base_size, 4] - what HotPath.prefilter_env_cube takes. taps: the sub-samples a side of an output texel (a power
    of two 1..16), None for hostmath.env_panorama_taps. out: a device tensor of 48 * base_size^2 bytes to write into, else one is
    allocated. One launch on the context's stream; nothing is synchronised or read back."""
    width, height, base = int(width), int(height), int(base_size)
    if taps is None:
        taps = hostmath.env_panorama_taps(width, height, base)
    taps = int(taps)
    if int(hp._L.ur_host_env_panorama_taps(width, height, base)) == 0 or taps not in (1, 2, 4, 8, 16):
        raise ValueError(f"no panorama build: {width} x {height} to base size {base} with {taps} taps a side (1..16384 x 1..8192; powers of two, 1..2048 and 1..16)")
    need = 4 * width * height
    with tensors.on_stream(hp):
        src = tensors.device_bytes(rgbe, need, hp.device, lambda have: f"a panorama of {width} x {height} RGBE texels is {need} bytes, the source has {have}")
        dst = out if out is not None else torch.empty((6, base, base, 4), dtype=torch.int16, device=src.device)
    if nbytes(dst) != 48 * base * base:
        raise ValueError(f"the top level of a cube of base size {base} is {48 * base * base} bytes, out has {nbytes(dst)}")
    _lib.check(hp._L.ur_env_panorama(hp._ctx, _ptr(src), need, width, height, base, taps, _ptr(dst), nbytes(dst)), "ur_env_panorama")
    dst._keep = src  # (the launch is still in flight)
    return dst


def bake_panorama(hp, rgbe, width: int, height: int, base_size: int, sample_count: int = 1024, taps=None, *, out=None) -> torch.Tensor:
    """panorama_to_cube chained into HotPath.prefilter_env_cube and HotPath.build_env_cube: a panorama's RGBE texels become the staged cube
    make_tables takes, with log2(base_size) + 1 mips, all on the device. out: as in HotPath.build_env_cube."""
    top = panorama_to_cube(hp, rgbe, width, height, base_size, taps)
    payload = hp.prefilter_env_cube(top, int(base_size), sample_count)
    return hp.build_env_cube(payload.view(torch.uint8).reshape(-1), _lib.UR_ENV_SOURCE_RGBA16F, int(base_size), int(base_size).bit_length(), out=out)


def sky_to_cube(hp, sky, base_size: int, taps: int = 1, *, out=None) -> torch.Tensor:
    """ur_env_sky: the procedural sky of the frame's sky pass for the lib.SkyConstants `sky` (only CameraPosition[1], LightDirection and
    LightColor are read) becomes the top level of an HDR cube: six RGBA16F faces of edge base_size as an int16 device tensor
    [6, base_size, base_size, 4] - what HotPath.prefilter_env_cube takes. taps: the sub-samples a side of an output texel (a power of two
    1..16). out: a device tensor of 48 * base_size^2 bytes to write into, else one is allocated. One launch on the context's stream;
    nothing is synchronised or read back."""
    base, taps = int(base_size), int(taps)
    if not isinstance(sky, _lib.SkyConstants):
        raise TypeError(f"sky is a lib.SkyConstants, not {type(sky).__name__}")
    if base < 1 or base > _lib.UR_ENV_SKY_MAX_BASE_SIZE or base & (base - 1) or taps not in (1, 2, 4, 8, 16):
        raise ValueError(f"no sky capture: base size {base} with {taps} taps a side (powers of two, 1..2048 and 1..16)")
    hostmath.env_sky_params(sky)  # (ValueError for constants the capture refuses)
    with tensors.on_stream(hp):
        dst = out if out is not None else torch.empty((6, base, base, 4), dtype=torch.int16, device=f"cuda:{hp.device}")
    if nbytes(dst) != 48 * base * base:
        raise ValueError(f"the top level of a cube of base size {base} is {48 * base * base} bytes, out has {nbytes(dst)}")
    _lib.check(hp._L.ur_env_sky(hp._ctx, C.byref(sky), base, taps, _ptr(dst), nbytes(dst)), "ur_env_sky")
    return dst


def bake_sky(hp, sky, base_size: int, sample_count: int = 1024, taps: int = 1, *, out=None) -> torch.Tensor:
    """sky_to_cube chained into HotPath.prefilter_env_cube and HotPath.build_env_cube: the sky of `sky` becomes the staged cube make_tables
    takes, with log2(base_size) + 1 mips, all on the device. out: as in HotPath.build_env_cube."""
    top = sky_to_cube(hp, sky, base_size, taps)
    payload = hp.prefilter_env_cube(top, int(base_size), sample_count)
    return hp.build_env_cube(payload.view(torch.uint8).reshape(-1), _lib.UR_ENV_SOURCE_RGBA16F, int(base_size), int(base_size).bit_length(), out=out)


def brdf_lut(hp, width: int = 128, height: int = 32, sample_count: int = 1024, *, out=None) -> torch.Tensor:
    """ur_brdf_lut: the split-sum BRDF table as a uint16 device tensor [height, width, 2] (scale, bias as UNORM16) - what
    make_tables takes in place of assets.load_brdf_lut_dds's; 128 x 32 is what the streaming lighting kernel requires. The sample table
    (hostmath.brdf_lut_table) is made and uploaded here. out: a device tensor of 4 * width * height bytes to write into, else one is
    allocated. One launch on the context's stream; nothing is synchronised or read back."""
    width, height, samples = int(width), int(height), int(sample_count)
    if not 1 <= width <= _lib.UR_BRDF_LUT_MAX_WIDTH or int(hp._L.ur_brdf_lut_table_bytes(height, samples)) == 0:
        raise ValueError(f"no BRDF LUT: {width} x {height} with {samples} samples (1..1024 x 1..256; a power of two, 16..4096)")
    with tensors.on_stream(hp):
        table = tensors.to_device(hostmath.brdf_lut_table(height, samples).copy(), hp.device)
        dst = out if out is not None else torch.empty((height, width, 2), dtype=torch.uint16, device=table.device)
    if nbytes(dst) != 4 * width * height:
        raise ValueError(f"a BRDF LUT of {width} x {height} is {4 * width * height} bytes, out has {nbytes(dst)}")
    _lib.check(hp._L.ur_brdf_lut(hp._ctx, width, height, samples, _ptr(table), nbytes(table), _ptr(dst), nbytes(dst)), "ur_brdf_lut")
    dst._keep = table  # (the launch is still in flight)
    return dst
