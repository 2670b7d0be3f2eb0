"""Caller-side constants for the hot path: thin Python over the C++ host math (include/ur_host.h), plus the camera /
light presets of the reference's shipped scenes (Assets/Scenes/{sponza,Duck,pica_pica}.json).

Everything numeric is computed by libur_hotpath.so (csrc/host_math.cpp); this module only marshals.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field

import numpy as np

from . import lib as _lib
from .payload import host_bytes


def _f(*v) -> np.ndarray:
    return np.asarray(v, dtype=np.float32).reshape(-1).copy()


def look_to_lh(eye, direction, up=(0.0, 1.0, 0.0)) -> np.ndarray:
    out = np.zeros(16, np.float32)
    _lib.load().ur_host_look_to_lh(_lib.fptr(_f(*eye)), _lib.fptr(_f(*direction)), _lib.fptr(_f(*up)), _lib.fptr(out))
    return out


def reverse_z_projection(fov_y: float, aspect: float, near: float = 0.1) -> np.ndarray:
    out = np.zeros(16, np.float32)
    _lib.load().ur_host_reverse_z_projection(fov_y, aspect, near, _lib.fptr(out))
    return out


def mat_mul(a, b) -> np.ndarray:
    out = np.zeros(16, np.float32)
    _lib.load().ur_host_mat_mul(_lib.fptr(_f(*a)), _lib.fptr(_f(*b)), _lib.fptr(out))
    return out


def mat_inverse(m) -> np.ndarray:
    out = np.zeros(16, np.float32)
    if not _lib.load().ur_host_mat_inverse(_lib.fptr(_f(*m)), _lib.fptr(out)):
        raise ValueError("singular matrix")
    return out


def frustum_planes(view_proj) -> np.ndarray:
    """BuildFrustumPlanesFromMatrix: 24 floats, also the planes of an extra cull view (ur_cull_view.planes). A light's view:
    frustum_planes(light_view_projection(fc.scene_center, fc.scene_radius, fc.light_direction))."""
    out = np.zeros(24, np.float32)
    _lib.load().ur_host_frustum_planes(_lib.fptr(_f(*view_proj)), _lib.fptr(out))
    return out


def is_aabb_in_frustum(planes, bmin, bmax) -> bool:
    return bool(_lib.load().ur_host_is_aabb_in_frustum(_lib.fptr(_f(*planes)), _lib.fptr(_f(*bmin)), _lib.fptr(_f(*bmax))))


def light_view_projection(center, radius: float, light_dir) -> np.ndarray:
    out = np.zeros(16, np.float32)
    _lib.load().ur_host_light_view_projection(_lib.fptr(_f(*center)), radius, _lib.fptr(_f(*light_dir)), _lib.fptr(out))
    return out


def taa_jitter(sample_index: int) -> np.ndarray:
    """BuildTaaJitter: the sub-pixel offset (x, y) of TemporalAA sample `sample_index` (the renderer's runs 0..7), fp32."""
    out = np.zeros(2, np.float32)
    _lib.load().ur_host_taa_jitter(sample_index, _lib.fptr(out))
    return out


def srgb_encode_table() -> np.ndarray:
    """ur_host_srgb_encode_table: the 255 ascending fp32 thresholds of the GBuffer resolve's sRGB encode (code = the number of entries
    with x >= entry)."""
    out = np.zeros(255, np.float32)
    _lib.load().ur_host_srgb_encode_table(_lib.fptr(out))
    return out


def srgb_decode_table() -> np.ndarray:
    """ur_host_srgb_decode_table: the 256 fp32 linear values of the sRGB codes 0..255, the textured GBuffer resolve's texel decode."""
    out = np.zeros(256, np.float32)
    _lib.load().ur_host_srgb_decode_table(_lib.fptr(out))
    return out


def bc_chain_bytes(format: int, width: int, height: int, mips: int) -> int:
    """ur_host_bc_chain_bytes: the bytes of a chain of `mips` BC1 / BC3 / BC5 levels as ur_texture2d lays them out (0 for anything it does not
    describe: another format, a dimension outside 1..65535, mips outside 1..255)."""
    return int(_lib.load().ur_host_bc_chain_bytes(int(format), int(width), int(height), int(mips)))


def bc_decode_level(format: int, blocks, level_width: int, level_height: int) -> np.ndarray:
    """ur_host_bc_decode_level: one level of ((w + 3) >> 2) x ((h + 3) >> 2) blocks (bytes or a uint8 array) -> its (h, w, 4) uint8 RGBA8 code
    words, by the functions the kernels decode with (csrc/bc_decode.h)."""
    data = host_bytes(blocks)
    per = 8 if format in (_lib.UR_TEXTURE_BC1_UNORM, _lib.UR_TEXTURE_BC1_UNORM_SRGB) else 16
    need = ((level_width + 3) >> 2) * ((level_height + 3) >> 2) * per
    if level_width < 1 or level_height < 1 or data.size < need:
        raise ValueError(f"a {level_width} x {level_height} level of format {format} needs {need} bytes of blocks, got {data.size}")
    out = np.zeros((level_height, level_width, 4), np.uint8)
    rc = _lib.load().ur_host_bc_decode_level(int(format), data.ctypes.data_as(C.c_void_p), int(level_width), int(level_height), out.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise ValueError(f"ur_host_bc_decode_level failed ({rc}): format {format}")
    return out


def texture_chain_bytes(format: int, width: int, height: int, mips: int) -> int:
    """ur_host_texture_chain_bytes: the bytes of a source chain of ur_texture_transcode, over its ten formats (71, 72, 74, 75, 77, 78, 80, 83,
    98, 99); 0 for anything else, as bc_chain_bytes."""
    return int(_lib.load().ur_host_texture_chain_bytes(int(format), int(width), int(height), int(mips)))


def texture_decode_level(format: int, blocks, level_width: int, level_height: int) -> np.ndarray:
    """ur_host_texture_decode_level: bc_decode_level over the ten source formats, by the functions the transcode kernel decodes with
    (csrc/bc_wide_decode.h)."""
    data = host_bytes(blocks)
    need = texture_chain_bytes(format, max(level_width, 1), max(level_height, 1), 1)
    if level_width < 1 or level_height < 1 or need == 0 or data.size < need:
        raise ValueError(f"a {level_width} x {level_height} level of format {format} needs {need} bytes of blocks, got {data.size}")
    out = np.zeros((level_height, level_width, 4), np.uint8)
    rc = _lib.load().ur_host_texture_decode_level(int(format), data.ctypes.data_as(C.c_void_p), int(level_width), int(level_height), out.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise ValueError(f"ur_host_texture_decode_level failed ({rc}): format {format}")
    return out


def lod_table() -> np.ndarray:
    """ur_host_lod_table: the 127 ascending fp32 thresholds 2^(j / 128), j = 1..127, of the textured GBuffer resolve's level of detail."""
    out = np.zeros(127, np.float32)
    _lib.load().ur_host_lod_table(_lib.fptr(out))
    return out


def apply_taa_jitter(proj, jitter, width: float, height: float) -> np.ndarray:
    """A copy of the projection with _31 += 2 jx / width, _32 += 2 jy / height (elements 8 and 9), as the reference jitters it."""
    out = _f(*proj)
    _lib.load().ur_host_apply_taa_jitter(_lib.fptr(out), _lib.fptr(_f(*jitter)), float(width), float(height))
    return out


def debug_font():
    """The built-in debug-print font (ur_host_debug_font): (atlas, glyphs, first_char, char_count) - atlas a (64, 64) uint8 array
    (R8), glyphs a (96, 10) float32 array of ur_debug_glyph records {UvMin, UvMax, Size, Offset, Advance, Padding} indexed by code,
    filled for codes first_char .. first_char + char_count - 1 = 32 .. 95."""
    L = _lib.load()
    info = (C.c_uint32 * 4)()
    _lib.check(L.ur_host_debug_font(None, 0, None, 0, info), "ur_host_debug_font")
    aw, ah, first, count = (int(v) for v in info)
    atlas = np.zeros((ah, aw), np.uint8)
    glyphs = np.zeros((first + count, 10), np.float32)
    _lib.check(L.ur_host_debug_font(atlas.ctypes.data_as(C.c_void_p), atlas.size, glyphs.ctypes.data_as(C.c_void_p), glyphs.shape[0], info),
               "ur_host_debug_font")
    return atlas, glyphs, first, count


def pack_culling_constants(view, proj, model_count: int, hzb_enabled: bool, hzb_mip_count: int, hzb_width: int,
                           hzb_height: int, debug_print: bool = False) -> np.ndarray:
    out = np.zeros(_lib.UR_CULL_CONSTANT_DWORDS, np.uint32)
    _lib.load().ur_host_pack_culling_constants(_lib.fptr(_f(*view)), _lib.fptr(_f(*proj)), model_count, int(hzb_enabled),
                                               hzb_mip_count, hzb_width, hzb_height, int(debug_print),
                                               out.ctypes.data_as(C.POINTER(C.c_uint32)))
    return out


def direction_from_euler_degrees(pitch: float, yaw: float) -> np.ndarray:
    out = np.zeros(3, np.float32)
    _lib.load().ur_host_direction_from_euler_degrees(pitch, yaw, _lib.fptr(out))
    return out


def camera_forward_from_euler_degrees(pitch: float, yaw: float) -> np.ndarray:
    out = np.zeros(3, np.float32)
    _lib.load().ur_host_camera_forward_from_euler_degrees(pitch, yaw, _lib.fptr(out))
    return out


def light_direction_roundtrip(json_dir) -> np.ndarray:
    out = np.zeros(3, np.float32)
    _lib.load().ur_host_light_direction_roundtrip(_lib.fptr(_f(*json_dir)), _lib.fptr(out))
    return out


@dataclass
class ScenePreset:
    """Camera/light values copied from Assets/Scenes/*.json; bounds as the renderer derives them (RendererUtils.cpp:46-82,
    277-286,533-540: per-model sphere bounds -> scene box -> centre/radius)."""
    name: str
    camera_position: tuple
    camera_rotation_deg: tuple | None = None  # (pitch, yaw, roll)
    camera_look_at: tuple | None = None
    fov_y_deg: float = 60.0
    light_rotation_deg: tuple | None = None
    light_direction: tuple | None = None
    light_intensity: float = 1.0
    light_color: tuple = (1.0, 1.0, 1.0)
    # world AABB of the scene's models (min, max); Sponza: accessor min/max of Assets/sponza/untitled.gltf through the
    # node's +90deg X rotation, LH z flip (GltfLoader.cpp:823), scale 0.01, translate (5,0,0) (sponza.json)
    model_aabb: tuple = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
    instance_count: int = 1
    # scene centre / radius as CreateSceneModelsFromJson derives them (union of per-command spheres); values produced by
    # ur_scene_extract (csrc/scene.cpp) on the shipped scene files and pinned by tests/test_scene.py
    scene_center: tuple | None = None
    scene_radius: float | None = None


SCENES = {
    "sponza": ScenePreset("sponza", (14.327, 0.762, 0.571), camera_rotation_deg=(-12.6, 261.8, 0.0), fov_y_deg=60.0,
                          light_rotation_deg=(-75.0, 0.0, 0.0), light_intensity=1.0, light_color=(1.0, 1.0, 1.0),
                          model_aabb=((-14.209459, -1.264425, -11.054260), (22.999081, 14.294332, 11.828071)), instance_count=25,
                          scene_center=(4.3948116, 6.5149517, 0.38690376), scene_radius=40.15736),
    "duck": ScenePreset("duck", (0.0, 1.5, 4.0), camera_look_at=(0.0, 1.0, 0.0), fov_y_deg=60.0,
                        light_direction=(-0.5, -1.0, -0.3), light_intensity=3.0, light_color=(1.0, 0.95, 0.9),
                        model_aabb=((-0.692985, 0.09929369, -0.539252), (0.96179897, 1.6396999, 0.61328197)), instance_count=1,
                        scene_center=(0.13440704, 0.8694968, 0.03701496), scene_radius=2.1976402),
    "pica_pica": ScenePreset("pica_pica", (-13.482, 20.457, -42.455), camera_rotation_deg=(19.199, 16.599, 0.0), fov_y_deg=60.0,
                             light_rotation_deg=(-45.0, -135.0, 0.0), light_intensity=1.0, light_color=(1.0, 0.95, 0.9),
                             model_aabb=((-36.92157, -1.1695042, -18.168373), (27.365425, 18.529217, 32.19241)), instance_count=170,
                             scene_center=(-3.2157097, 3.8195744, 1.1750641), scene_radius=62.74809),
}


@dataclass
class FrameConstants:
    width: int
    height: int
    view: np.ndarray
    proj: np.ndarray
    camera_position: np.ndarray
    light_direction: np.ndarray
    scene: _lib.SceneConstants
    sky: _lib.SkyConstants
    scene_center: np.ndarray
    scene_radius: float
    sky_radius: float
    near: float = 0.1
    extra: dict = field(default_factory=dict)


def build_frame_constants(preset: ScenePreset | str, width: int, height: int, *, shadow_strength: float = 1.0,
                          shadow_bias: float = 0.0, shadow_size: int = 2048, env_mip_count: int = 9,
                          near: float = 0.1) -> FrameConstants:
    """What FApplication/FDeferredRenderer compute per frame before recording the four passes."""
    if isinstance(preset, str):
        preset = SCENES[preset]
    L = _lib.load()
    pos = _f(*preset.camera_position)
    if preset.camera_look_at is not None:
        d = _f(*preset.camera_look_at) - pos
        fwd = (d / np.float32(np.sqrt(np.float32((d * d).sum())))).astype(np.float32)
    else:
        fwd = camera_forward_from_euler_degrees(preset.camera_rotation_deg[0], preset.camera_rotation_deg[1])
    view = look_to_lh(pos, fwd)
    proj = reverse_z_projection(math.radians(preset.fov_y_deg), width / height, near)
    if preset.light_direction is not None:
        jd = _f(*preset.light_direction)
    else:
        jd = direction_from_euler_degrees(preset.light_rotation_deg[0], preset.light_rotation_deg[1])
    light_dir = light_direction_roundtrip(jd)
    if preset.scene_center is not None and preset.scene_radius is not None:
        center, scene_radius = _f(*preset.scene_center), float(preset.scene_radius)
    else:  # one model sphere (centre of the AABB, half its diagonal, >= 1) -> box -> centre / radius
        mn, mx = _f(*preset.model_aabb[0]), _f(*preset.model_aabb[1])
        center = ((mn + mx) * np.float32(0.5)).astype(np.float32)
        model_radius = max(float(np.sqrt(((mx - mn) ** 2).sum())) * 0.5, 1.0)
        scene_radius = max(float(np.sqrt(3.0 * (2.0 * model_radius) ** 2)) * 0.5, 1.0)
    sky_radius = max(scene_radius * 5.0, 100.0)  # DeferredRenderer.cpp:349
    lvp = light_view_projection(center, scene_radius, light_dir)
    scene = _lib.SceneConstants()
    L.ur_host_fill_scene_constants(_lib.fptr(view), _lib.fptr(proj), _lib.fptr(pos), preset.light_intensity, _lib.fptr(light_dir),
                                   _lib.fptr(_f(*preset.light_color)), _lib.fptr(lvp), shadow_strength, shadow_bias,
                                   float(shadow_size), float(shadow_size), float(env_mip_count), C.byref(scene))
    sky = _lib.SkyConstants()
    L.ur_host_fill_sky_constants(_lib.fptr(view), _lib.fptr(proj), _lib.fptr(pos), sky_radius, _lib.fptr(light_dir),
                                 _lib.fptr(_f(*preset.light_color)), C.byref(sky))
    return FrameConstants(width, height, view, proj, pos, light_dir, scene, sky, center, scene_radius, sky_radius, near)


def mesh_primitive(vertex_count: int, position, indices, *, normal=None, texcoord=None, tangent=None, color=None, color_components: int = 3, mode: int = 4):
    """A ur_mesh_primitive (include/ur_mesh.h). A stream is (byte offset, stride) or None for an absent one; a stride of None or 0 is the
    packed default (12, 12, 8, 16 and 4 * color_components bytes). indices is (byte offset, count, component type 5121 / 5123 / 5125)."""
    p = _lib.MeshPrimitive()
    packed = {"position": 12, "normal": 12, "texcoord": 8, "tangent": 16, "color": 4 * int(color_components)}
    for name, stream in (("position", position), ("normal", normal), ("texcoord", texcoord), ("tangent", tangent), ("color", color)):
        if stream is not None:
            offset, stride = stream
            setattr(p, name, _lib.MeshStream(int(offset), int(stride) if stride else packed[name], 1))
    p.index_offset, p.index_count, p.index_component_type = int(indices[0]), int(indices[1]), int(indices[2])
    p.mode, p.vertex_count, p.color_components = int(mode), int(vertex_count), int(color_components)
    return p


def mesh_primitive_array(primitives):
    """A ctypes array of ur_mesh_primitive from MeshPrimitive records (copied)."""
    primitives = list(primitives)
    return (_lib.MeshPrimitive * max(len(primitives), 1))(*primitives)


def mesh_layout(primitives, buffer_size: int):
    """ur_mesh_layout_of: (lib.MeshLayout, [(vertex_offset, index_start, index_count) per primitive]); ValueError with the library's text
    for anything it refuses."""
    primitives = list(primitives)
    layout, sections = _lib.MeshLayout(), (_lib.MeshSection * max(len(primitives), 1))()
    rc = _lib.load().ur_mesh_layout_of(mesh_primitive_array(primitives), len(primitives), int(buffer_size), C.byref(layout), sections)
    if rc != 0:
        raise ValueError(_lib.load().ur_last_error().decode(errors="replace"))
    return layout, [(s.vertex_offset, s.index_start, s.index_count) for s in sections[:len(primitives)]]


def mesh_build(buffer, primitives):
    """ur_host_mesh_build: the mesh rule on the host, serial, by the functions the kernels run (csrc/mesh_rule.h). `buffer`:
    the .bin's bytes. Returns (vertices uint32[V, 16], indices uint32[I], sections, lib.MeshInfo): the bytes HotPath.build_mesh leaves on
    the device."""
    primitives = list(primitives)
    data = host_bytes(buffer)
    layout, sections = mesh_layout(primitives, data.size)
    vertices, indices, info = np.zeros((layout.vertex_count, 16), np.uint32), np.zeros(layout.index_count, np.uint32), _lib.MeshInfo()
    rc = _lib.load().ur_host_mesh_build(data.ctypes.data_as(C.c_void_p), data.size, mesh_primitive_array(primitives), len(primitives),
                                        vertices.ctypes.data_as(C.c_void_p), indices.ctypes.data_as(C.c_void_p), None, C.byref(info))
    if rc != 0:
        raise ValueError(f"ur_host_mesh_build failed ({rc})")
    return vertices, indices, sections, info


def scene_build(nodes, meshes, mesh_infos, materials, draws, frame, slot_count: int, constants_stride: int = 608, constants_address: int = 0, *,
                transforms_only: bool = False, out=None, library=None):
    """ur_host_scene_build: the scene rule on the host, serial, by the functions the kernels run (csrc/scene_rule.h). The
    tables are numpy arrays of the records' bytes (any dtype); `frame` a lib.SceneConstants. Returns a dict of numpy arrays: bounds float32
    [D, 2, 4], commands uint32 [D, 16], constants uint8 [slot_count, constants_stride], centers float32 [D, 4], summary uint8 [48] (a
    lib.SceneBuildSummary) - the bytes HotPath.build_scene leaves on the device when its constants lie at constants_address. out: such a
    dict to write into (what a build leaves alone keeps its bytes), else zeroed arrays."""
    L = library if library is not None else _lib.load()
    tables = [host_bytes(t, reinterpret=True) for t in (nodes, meshes, mesh_infos, materials, draws)]
    counts = [t.size // C.sizeof(r) for t, r in zip(tables, (_lib.SceneNode, _lib.SceneMesh, _lib.MeshInfo, _lib.SceneMaterialFactors, _lib.SceneDraw))]
    if counts[1] != counts[2]:
        raise ValueError(f"{counts[1]} mesh records and {counts[2]} info records")
    D = counts[4]
    if out is None:
        out = {"bounds": np.zeros((D, 2, 4), np.float32), "commands": np.zeros((D, 16), np.uint32), "constants": np.zeros((slot_count, constants_stride), np.uint8),
               "centers": np.zeros((D, 4), np.float32), "summary": np.zeros(48, np.uint8)}
    at = lambda a: a.ctypes.data  # noqa: E731
    record = _lib.SceneBuildTables(at(tables[0]), at(tables[1]), at(tables[2]), at(tables[3]), at(tables[4]), counts[0], counts[1], counts[3], D)
    outputs = _lib.SceneBuildOutputs(at(out["bounds"]), at(out["commands"]), at(out["constants"]), at(out["centers"]) if out.get("centers") is not None else None,
                                     at(out["summary"]), constants_stride, slot_count)
    rc = L.ur_host_scene_build(C.byref(record), C.byref(frame), C.byref(outputs), C.c_uint64(constants_address), C.c_uint32(1 if transforms_only else 0))
    if rc != 0:
        raise ValueError(f"ur_host_scene_build failed ({rc})")
    return out


def _aligned16(nbytes: int) -> np.ndarray:
    """nbytes uint8 at a 16-byte aligned address (a view into a larger array)."""
    raw = np.zeros(nbytes + 16, np.uint8)
    start = (-raw.ctypes.data) % 16
    return raw[start:start + nbytes]


def env_cube_build(payload, format: int, base: int, mips: int, *, library=None):
    """ur_host_env_cube_build: the environment cube build on the host, serial, by the decoder the kernels run
    (csrc/bc6h_decode.h) and the staging ur_stage_env_cube runs. payload: the DDS cube's payload (bytes or a uint8 array;
    assets.load_env_cube_dds_source). Returns (the staged cube as uint16 [texels, 4] - the bytes HotPath.build_env_cube leaves on the
    device - and the number of reserved-mode blocks)."""
    L = library if library is not None else _lib.load()
    data = host_bytes(payload)
    texels = int(_lib.load().ur_env_cube_texels(int(base), int(mips)))
    src = _aligned16(data.size)
    src[:] = data
    dst = _aligned16(8 * texels)
    bad = C.c_uint32(0)
    rc = L.ur_host_env_cube_build(C.c_void_p(src.ctypes.data), C.c_size_t(data.size), C.c_uint32(int(format)), C.c_uint32(int(base)), C.c_uint32(int(mips)),
                                  C.c_void_p(dst.ctypes.data), C.c_size_t(texels), C.byref(bad))
    if rc != 0:
        raise ValueError(f"ur_host_env_cube_build failed ({rc}): format {format}, base size {base}, {mips} mips, {data.size} payload bytes")
    return dst.view(np.uint16).reshape(texels, 4), int(bad.value)


def env_prefilter_table(base: int, sample_count: int, *, library=None) -> np.ndarray:
    """ur_host_env_prefilter_table: the sample table of the environment prefilter for a cube of edge `base` and
    `sample_count` samples a texel, as uint8 at a 16-byte aligned address - the bytes HotPath.prefilter_env_cube uploads. ValueError for a
    base that is no power of two up to 2048 or a sample count that is no power of two in 16..4096."""
    L = library if library is not None else _lib.load()
    need = int(_lib.load().ur_env_prefilter_table_bytes(int(base), int(sample_count)))
    if need == 0:
        raise ValueError(f"no prefilter table: base size {base}, {sample_count} samples (powers of two, 1..2048 and 16..4096)")
    out = _aligned16(need)
    rc = L.ur_host_env_prefilter_table(C.c_uint32(int(base)), C.c_uint32(int(sample_count)), C.c_void_p(out.ctypes.data), C.c_size_t(need))
    if rc != 0:
        raise ValueError(f"ur_host_env_prefilter_table failed ({rc})")
    return out


def env_prefilter(src, base: int, sample_count: int = 1024, *, table=None, library=None) -> np.ndarray:
    """ur_host_env_prefilter: the environment prefilter on the host, serial, by the functions the kernels run
    (csrc/env_prefilter_rule.h). src: the cube's top level, six RGBA16F faces (6 * base * base * 8 bytes, any dtype or bytes;
    assets.load_env_cube_top_level). Returns the prefiltered chain as uint16 [texels, 4] in DDS order - the bytes
    HotPath.prefilter_env_cube leaves on the device, the UR_ENV_SOURCE_RGBA16F payload of env_cube_build with log2(base) + 1 mips."""
    L = library if library is not None else _lib.load()
    data = host_bytes(src, reinterpret=True)
    if table is None:
        table = env_prefilter_table(base, sample_count, library=library)
    mips = int(base).bit_length()
    need = int(_lib.load().ur_env_cube_source_bytes(_lib.UR_ENV_SOURCE_RGBA16F, int(base), mips))
    source = _aligned16(data.size)
    source[:] = data
    tab = _aligned16(table.size)
    tab[:] = host_bytes(table, reinterpret=True)
    dst = _aligned16(need)
    rc = L.ur_host_env_prefilter(C.c_void_p(source.ctypes.data), C.c_size_t(data.size), C.c_uint32(int(base)), C.c_uint32(int(sample_count)),
                                 C.c_void_p(tab.ctypes.data), C.c_size_t(tab.size), C.c_void_p(dst.ctypes.data), C.c_size_t(need))
    if rc != 0:
        raise ValueError(f"ur_host_env_prefilter failed ({rc}): base size {base}, {sample_count} samples, {data.size} source bytes, {tab.size} table bytes")
    return dst.view(np.uint16).reshape(-1, 4)


def env_panorama_taps(width: int, height: int, base: int) -> int:
    """ur_host_env_panorama_taps: the taps a side recommended for a width x height panorama and a cube of edge `base`: the
    smallest power of two K with 3 K base >= 2 width and 3 K base >= 4 height, at most 16. ValueError for sizes the build refuses."""
    taps = int(_lib.load().ur_host_env_panorama_taps(int(width), int(height), int(base)))
    if taps == 0:
        raise ValueError(f"no panorama build: {width} x {height} to base size {base} (1..16384 x 1..8192; a power of two, 1..2048)")
    return taps


def env_panorama(rgbe, width: int, height: int, base: int, taps=None, *, library=None) -> np.ndarray:
    """ur_host_env_panorama: the environment from a panorama on the host, serial, by the functions the kernel runs
    (csrc/env_panorama_rule.h). rgbe: the panorama's texels, four bytes R G B E each, top row first (4 * width * height bytes:
    assets.load_panorama_hdr). taps: the sub-samples a side, None for env_panorama_taps. Returns the cube's top level as uint16
    [6, base, base, 4] - the bytes environment.panorama_to_cube leaves on the device, the source of env_prefilter."""
    L = library if library is not None else _lib.load()
    data = host_bytes(rgbe)
    if taps is None:
        taps = env_panorama_taps(width, height, base)
    source = _aligned16(data.size)
    source[:] = data
    need = 48 * int(base) * int(base) if 0 < int(base) <= 2048 else 0
    dst = _aligned16(need)
    rc = L.ur_host_env_panorama(C.c_void_p(source.ctypes.data), C.c_size_t(data.size), C.c_uint32(int(width)), C.c_uint32(int(height)), C.c_uint32(int(base)),
                                C.c_uint32(int(taps)), C.c_void_p(dst.ctypes.data), C.c_size_t(need))
    if rc != 0:
        raise ValueError(f"ur_host_env_panorama failed ({rc}): {width} x {height} to base size {base}, {taps} taps a side, {data.size} source bytes")
    return dst.view(np.uint16).reshape(6, int(base), int(base), 4)


def env_sky_params(sky) -> np.ndarray:
    """ur_host_env_sky_params: the ten fp32 values the sky capture folds a lib.SkyConstants to, in float64 rounded once:
    the normalised sun direction [0:3], the Rayleigh term [3:6], the Mie term [6:9], the sun attenuation [9]. ValueError for a
    CameraPosition[1], LightDirection or LightColor that is not finite or a LightDirection of length zero."""
    out = np.zeros(10, np.float32)
    rc = _lib.load().ur_host_env_sky_params(C.byref(sky), _lib.fptr(out))
    if rc != 0:
        raise ValueError(f"ur_host_env_sky_params failed ({rc}): CameraPosition.y, LightDirection and LightColor are finite, LightDirection is not zero")
    return out


def env_sky(sky, base: int, taps: int = 1, *, library=None) -> np.ndarray:
    """ur_host_env_sky: the sky capture on the host, serial, by the functions the kernel runs (csrc/env_sky_rule.h). Returns
    the cube's top level as uint16 [6, base, base, 4] - the bytes environment.sky_to_cube leaves on the device, the source of
    env_prefilter."""
    L = library if library is not None else _lib.load()
    need = 48 * int(base) * int(base) if 0 < int(base) <= 2048 else 0
    dst = _aligned16(need)
    rc = L.ur_host_env_sky(C.byref(sky), C.c_uint32(int(base)), C.c_uint32(int(taps)), C.c_void_p(dst.ctypes.data), C.c_size_t(need))
    if rc != 0:
        raise ValueError(f"ur_host_env_sky failed ({rc}): base size {base}, {taps} taps a side")
    return dst.view(np.uint16).reshape(6, int(base), int(base), 4)


def brdf_lut_table(height: int, sample_count: int, *, library=None) -> np.ndarray:
    """ur_host_brdf_lut_table: the sample table of the BRDF LUT for `height` rows and `sample_count` samples a texel, as
    uint8 at a 16-byte aligned address - the bytes environment.brdf_lut uploads. ValueError for a height outside 1..256 or a sample count
    that is no power of two in 16..4096."""
    L = library if library is not None else _lib.load()
    need = int(_lib.load().ur_brdf_lut_table_bytes(int(height), int(sample_count)))
    if need == 0:
        raise ValueError(f"no BRDF LUT table: {height} rows, {sample_count} samples (1..256; a power of two, 16..4096)")
    out = _aligned16(need)
    rc = L.ur_host_brdf_lut_table(C.c_uint32(int(height)), C.c_uint32(int(sample_count)), C.c_void_p(out.ctypes.data), C.c_size_t(need))
    if rc != 0:
        raise ValueError(f"ur_host_brdf_lut_table failed ({rc})")
    return out


def brdf_lut(width: int = 128, height: int = 32, sample_count: int = 1024, *, table=None, library=None) -> np.ndarray:
    """ur_host_brdf_lut: the BRDF LUT on the host, serial, by the functions the kernel runs (csrc/brdf_lut_rule.h). Returns
    uint16 [height, width, 2] (scale, bias) - the bytes environment.brdf_lut leaves on the device, what assets.load_brdf_lut_dds gives
    for the shipped file."""
    L = library if library is not None else _lib.load()
    if table is None:
        table = brdf_lut_table(height, sample_count, library=library)
    tab = _aligned16(table.size)
    tab[:] = host_bytes(table, reinterpret=True)
    need = 4 * int(width) * int(height) if 0 < int(width) <= 1024 and 0 < int(height) <= 256 else 0
    dst = _aligned16(need)
    rc = L.ur_host_brdf_lut(C.c_uint32(int(width)), C.c_uint32(int(height)), C.c_uint32(int(sample_count)), C.c_void_p(tab.ctypes.data), C.c_size_t(tab.size),
                            C.c_void_p(dst.ctypes.data), C.c_size_t(need))
    if rc != 0:
        raise ValueError(f"ur_host_brdf_lut failed ({rc}): {width} x {height}, {sample_count} samples, {tab.size} table bytes")
    return dst.view(np.uint16).reshape(int(height), int(width), 2)
