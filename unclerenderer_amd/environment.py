"""An environment from a lat-long Radiance .hdr panorama, on the device: functions over a HotPath.

    rgbe = assets.load_panorama_hdr(path)                          # the file's texels, uint8 [H, W, 4]
    cube = environment.bake_panorama(hp, rgbe, W, H, base_size)    # the staged cube make_tables takes, log2(base_size) + 1 mips

panorama_to_cube is the new step (ur_env_panorama: panorama -> the cube's top level); bake_panorama chains it into
HotPath.prefilter_env_cube and HotPath.build_env_cube. Everything runs on the context's stream; nothing is synchronised or read back."""
from __future__ import annotations

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
