"""Asset loading. IBL: DDS (BC6H cube, RG16 LUT) -> host arrays ready for HotPath.stage_env_cube / make_tables; or the cube's payload as it
lies (load_env_cube_dds_source) -> what HotPath.build_env_cube decodes and stages on the device; or a Radiance .hdr panorama's texels
(load_panorama_hdr) -> what environment.bake_panorama turns into the staged cube on the device. Material textures: DDS
(RGBA8, BC1, BC3, BC5) -> what hotpath.pack_texture / pack_texture_bc take; BC blocks stay compressed, the sampler decodes them.
BC2, BC4 and BC7 too (load_texture_dds_source) -> what HotPath.transcode_texture takes: decoded to RGBA8 once, on the device.
All parsing and decoding happens in libur_hotpath.so (csrc/dds.cpp, csrc/hdr.cpp); this module only reads the file and marshals."""
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


def load_env_cube_top_level(path) -> tuple[np.ndarray, int]:
    """Level 0 of any cube DDS load_env_cube_dds reads, as six RGBA16F faces: (texels uint16 [6, base, base, 4], base size) - the source
    of HotPath.prefilter_env_cube and hostmath.env_prefilter when base is a power of two."""
    texels, base, mips, _ = load_env_cube_dds(path)
    per_face = sum(max(1, base >> m) ** 2 for m in range(mips))
    return np.ascontiguousarray(texels.reshape(6, per_face, 4)[:, :base * base]).reshape(6, base, base, 4), base


def parse_panorama_hdr(data: bytes) -> _lib.HdrInfo:
    """ur_hdr_parse: the header of a Radiance .hdr file (width, height, where the payload starts, whether it is run-length coded).
    ValueError with the library's text for what it refuses."""
    info = _lib.HdrInfo()
    L = _lib.load()
    rc = L.ur_hdr_parse(data, len(data), C.byref(info))
    if rc != 0:
        raise ValueError(f"ur_hdr_parse failed ({rc}): {L.ur_hdr_last_error().decode(errors='replace')}")
    return info


def load_panorama_hdr(path_or_bytes) -> np.ndarray:
    """A lat-long Radiance .hdr panorama (a path, or the file's bytes) as its own texels: uint8 [height, width, 4], R G B E, top row first -
    the source of environment.panorama_to_cube / bake_panorama and hostmath.env_panorama. Run-length coded scanlines are expanded here, on
    the host (ur_hdr_unpack); the decode to numbers is the device's."""
    data = bytes(path_or_bytes) if isinstance(path_or_bytes, (bytes, bytearray, memoryview)) else Path(path_or_bytes).read_bytes()
    info = parse_panorama_hdr(data)
    out = np.zeros((int(info.height), int(info.width), 4), np.uint8)
    L = _lib.load()
    rc = L.ur_hdr_unpack(data, len(data), C.byref(info), out.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise ValueError(f"ur_hdr_unpack failed ({rc}): {L.ur_hdr_last_error().decode(errors='replace')}")
    return out


def load_env_cube_dds_source(path_or_bytes) -> tuple[np.ndarray, int, int, int]:
    """The source of HotPath.build_env_cube from a DDS file (a path, or the file's bytes): the payload behind the header as a uint8 array -
    BC6H blocks or RGBA16F texels, six faces, face-major with mips inner - with (format, base size, mip count): lib.UR_ENV_SOURCE_*.
    Nothing is decoded here. ValueError for what load_env_cube_dds refuses (no cube, an array of cubes, faces that are not square) and for
    a cube of any other format."""
    data = bytes(path_or_bytes) if isinstance(path_or_bytes, (bytes, bytearray, memoryview)) else Path(path_or_bytes).read_bytes()
    info = parse_dds(data)
    if not info.is_cube or info.slices != 6 or info.width != info.height:
        raise ValueError("not a single cube map")
    fmt, base, mips = int(info.dxgi_format), int(info.width), int(info.mip_count)
    size = int(_lib.load().ur_env_cube_source_bytes(fmt, base, mips))
    if size == 0:
        raise ValueError(f"a cube of format {fmt} with {mips} mips is no source of the environment cube build (10, 95, 96; up to 16 mips)")
    return np.frombuffer(data, np.uint8, size, int(info.header_size)).copy(), fmt, base, mips


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


def gltf_mesh_primitives(gltf: dict, mesh_index: int):
    """The hostmath.mesh_primitive records of meshes[mesh_index] of a parsed .gltf, and each primitive's material index (-1: none), as the
    reference's loader reads them (GltfLoader.cpp:732-801): a stream's offset is the accessor's byteOffset plus the view's, its stride the
    view's byteStride or the packed size, the mode 4 and the index component type 5125 by default. ValueError for a primitive without
    POSITION or indices, a sparse accessor or an attribute that is not fp32."""
    from . import hostmath
    accessors, views = gltf.get("accessors", []), gltf.get("bufferViews", [])

    def stream(index):
        a = accessors[index]
        if "sparse" in a or a.get("componentType", 5126) != 5126 or "bufferView" not in a:
            raise ValueError(f"accessor {index}: only plain fp32 attribute accessors are built (no sparse, normalised-integer or view-less ones)")
        view = views[a["bufferView"]]
        if view.get("buffer", 0) != 0:
            raise ValueError(f"accessor {index}: only buffers[0] is read")
        return (a.get("byteOffset", 0) + view.get("byteOffset", 0), view.get("byteStride", 0))

    primitives, materials = [], []
    for k, primitive in enumerate(gltf["meshes"][mesh_index]["primitives"]):
        attributes = primitive.get("attributes", {})
        if "POSITION" not in attributes or "indices" not in primitive:
            raise ValueError(f"mesh {mesh_index}, primitive {k}: POSITION and indices are required")
        streams = {name: stream(attributes[key]) for key, name in (("NORMAL", "normal"), ("TEXCOORD_0", "texcoord"), ("TANGENT", "tangent"), ("COLOR_0", "color"))
                   if key in attributes}
        components = 4 if "COLOR_0" in attributes and accessors[attributes["COLOR_0"]].get("type") == "VEC4" else 3
        a = accessors[primitive["indices"]]
        if "sparse" in a or "bufferView" not in a or views[a["bufferView"]].get("buffer", 0) != 0:
            raise ValueError(f"mesh {mesh_index}, primitive {k}: the index accessor needs a plain view of buffers[0]")
        indices = (a.get("byteOffset", 0) + views[a["bufferView"]].get("byteOffset", 0), a.get("count", 0), a.get("componentType", 5125))
        primitives.append(hostmath.mesh_primitive(accessors[attributes["POSITION"]].get("count", 0), stream(attributes["POSITION"]), indices,
                                                  color_components=components, mode=primitive.get("mode", 4), **streams))
        materials.append(int(primitive.get("material", -1)))
    return primitives, materials


def read_gltf(path):
    """(the parsed .gltf, the bytes of its external buffer). The buffer is the file buffers[0].uri names, beside the .gltf; a GLB file and
    an embedded (data:) buffer are refused."""
    import json
    path = Path(path)
    head = path.read_bytes()[:4]
    if head == b"glTF":
        raise ValueError(f"{path}: a binary glTF (GLB) is not read; export the .gltf with an external .bin")
    gltf = json.loads(path.read_text())
    buffers = gltf.get("buffers", [])
    uri = buffers[0].get("uri") if buffers else None
    if not uri:
        raise ValueError(f"{path}: buffers[0] has no uri (a GLB-stored buffer is not read)")
    if uri.startswith("data:"):
        raise ValueError(f"{path}: an embedded (data:) buffer is not read; export the .gltf with an external .bin")
    from urllib.parse import unquote
    return gltf, (path.parent / unquote(uri)).read_bytes()


def load_gltf_meshes(path, hp):
    """Every mesh of a .gltf built on the device: the external .bin is uploaded once and HotPath.build_mesh runs per glTF mesh, on the
    context's stream, nothing read back. Returns the hotpath.Mesh objects in the file's mesh order, each with `materials` (per primitive,
    the glTF material index). Which model draws which mesh, and the pipeline keys, stay ur_scene_extract's."""
    from . import hotpath
    gltf, data = read_gltf(path)
    with hotpath.tensors.on_stream(hp):  # (the buffer is dropped at return, the builds that read it still in flight on the context's stream)
        buffer = hotpath.tensors.to_device(np.frombuffer(data, np.uint8).copy(), hp.device)
    meshes = []
    for index in range(len(gltf.get("meshes", []))):
        primitives, materials = gltf_mesh_primitives(gltf, index)
        mesh = hp.build_mesh(buffer, primitives)
        mesh.materials = materials
        meshes.append(mesh)
    return meshes


def gltf_material_factors(gltf: dict) -> np.ndarray:
    """The lib.SceneMaterialFactors records of a parsed .gltf's materials (a structured array of len(materials) + 1 records), as the
    reference's loader and model set-up read them (GltfLoader.cpp:1040-1100, RendererUtils.cpp:34-44): baseColorFactor, metallicFactor,
    roughnessFactor (1), emissiveFactor (0), alphaMode MASK with alphaCutoff (0.5), and per texture the KHR_texture_transform offset,
    scale and rotation as (offset.xy, scale.xy) and (cos, sin, 0, 0), in fp32. The last record is the default material: what a primitive
    without a material gets (index -1), and every primitive of a file without materials, textures or images (the reference reads the
    materials only when all three are there)."""
    record = np.dtype(_lib.SceneMaterialFactors)
    materials = gltf.get("materials") or []
    out = np.zeros(len(materials) + 1, record)
    out["BaseColor"], out["BaseColorAlpha"], out["MetallicFactor"], out["RoughnessFactor"], out["AlphaCutoff"] = 1.0, 1.0, 1.0, 1.0, 0.5
    out["transforms"][:, 0::2] = (0.0, 0.0, 1.0, 1.0)
    out["transforms"][:, 1::2] = (1.0, 0.0, 0.0, 0.0)
    if not (materials and gltf.get("textures") and gltf.get("images")):
        return out

    def number(array, index, default):
        return array[index] if isinstance(array, list) and index < len(array) and isinstance(array[index], (int, float)) else default

    def transform(info):
        offset, scale, rotation = [0.0, 0.0], [1.0, 1.0], 0.0
        if isinstance(info, dict):
            source = (info.get("extensions") or {}).get("KHR_texture_transform") or info
            offset = [number(source.get("offset"), k, offset[k]) for k in range(2)]
            scale = [number(source.get("scale"), k, scale[k]) for k in range(2)]
            rotation = source.get("rotation", rotation)
        r = np.float32(rotation)
        return (offset[0], offset[1], scale[0], scale[1]), (np.cos(r), np.sin(r), 0.0, 0.0)

    for k, material in enumerate(materials):
        m = out[k]
        pbr = material.get("pbrMetallicRoughness")
        pairs = [transform(None)] * 4
        if isinstance(pbr, dict):
            factor = pbr.get("baseColorFactor")
            if isinstance(factor, list):
                m["BaseColor"] = [number(factor, c, 1.0) for c in range(3)]
                m["BaseColorAlpha"] = number(factor, 3, 1.0)
            m["MetallicFactor"], m["RoughnessFactor"] = pbr.get("metallicFactor", 1.0), pbr.get("roughnessFactor", 1.0)
            pairs[0], pairs[1] = transform(pbr.get("baseColorTexture")), transform(pbr.get("metallicRoughnessTexture"))
        pairs[2], pairs[3] = transform(material.get("normalTexture")), transform(material.get("emissiveTexture"))
        emissive = material.get("emissiveFactor")
        if isinstance(emissive, list):
            m["EmissiveFactor"] = [number(emissive, c, 0.0) for c in range(3)]
        if material.get("alphaMode") == "MASK":
            m["AlphaMode"], m["AlphaCutoff"] = 1, material.get("alphaCutoff", 0.5)
        for t, (offset_scale, rotation) in enumerate(pairs):
            m["transforms"][2 * t], m["transforms"][2 * t + 1] = offset_scale, rotation
    return out
