"""ctypes binding of the C-ABI (include/ur_hotpath.h, include/ur_raster.h, include/ur_mesh.h, include/ur_scene_build.h, include/ur_env_cube.h, include/ur_env_prefilter.h, include/ur_env_panorama.h, include/ur_env_sky.h, include/ur_brdf_lut.h, include/ur_host.h).

The shared library is the product; there is no Python or CPU fallback. If it is missing, importing the compute
entry points raises — build it with `python -m unclerenderer_amd.build` (hipcc, gfx950).
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import numpy as np

_LIB_PATH = Path(__file__).resolve().parent / "csrc" / "_build" / "libur_hotpath.so"
if os.environ.get("UR_HOTPATH_LIB"):  # diagnostic builds (e.g. the in-kernel-stamps build of tools/stamps_lighting.py)
    _LIB_PATH = Path(os.environ["UR_HOTPATH_LIB"]).resolve()

UR_OK = 0
UR_EINVAL, UR_EHIP, UR_ENOMEM, UR_ENODEVICE, UR_EUNSUPPORTED, UR_ETIMEOUT = -1, -2, -3, -4, -5, -6
UR_MAX_HZB_MIPS = 16
UR_CULL_CONSTANT_DWORDS = 46
UR_INDIRECT_COMMAND_STRIDE = 64
UR_INDIRECT_INSTANCE_COUNT_OFFSET = 44


# ur_set_option keys (include/ur_hotpath.h)
UR_OPT_LIGHTING_STREAM, UR_OPT_LIGHTING_WAVES_PER_WG, UR_OPT_LIGHTING_TILED_WAVES, UR_OPT_LIGHTING_LEAVE_CUS, UR_OPT_RIDE_WALKERS = 1, 2, 3, 4, 5
UR_OPT_CULL_STORE, UR_OPT_LIGHTING_BALANCE, UR_OPT_BALANCE_POOL_16THS, UR_OPT_BALANCE_CHUNK_SHIFT, UR_OPT_DEBUG_HZB_RIDE_STALL = 7, 8, 9, 10, 11
UR_OPT_TAA_TONEMAP_HISTORY_STORE = 12


class MipDesc(C.Structure):
    _fields_ = [("offset", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32)]


class DrawRanges(C.Structure):
    """ur_draw_ranges (include/ur_hotpath.h): per-range compacted draw commands and counts of ur_cull_indirect_args_draws."""
    _fields_ = [("offsets", C.c_void_p), ("range_count", C.c_uint32), ("commands", C.c_void_p), ("counts", C.c_void_p)]


UR_MAX_CULL_VIEWS = 4


class CullView(C.Structure):
    """ur_cull_view (include/ur_hotpath.h): one extra frustum-only view of ur_cull_indirect_args_views."""
    _fields_ = [("planes", C.c_float * 24), ("mask", C.c_void_p), ("visible_idx", C.c_void_p), ("visible_count", C.c_void_p),
                ("draws", C.POINTER(DrawRanges))]


class RasterDraws(C.Structure):
    """ur_raster_draws (include/ur_raster.h): the command slots of a raster pass and which of them to draw."""
    _fields_ = [("commands", C.c_void_p), ("command_count", C.c_uint32), ("visible_idx", C.c_void_p), ("visible_count", C.c_void_p),
                ("index_base", C.c_uint32), ("ranges", C.POINTER(DrawRanges))]


class FrameShadowPass(C.Structure):
    """ur_frame_shadow_pass (include/ur_frame.h): the draws, target and optional counters of UR_FRAME_SHADOW_PASS."""
    _fields_ = [("draws", RasterDraws), ("shadow_map", C.c_void_p), ("stats4", C.c_void_p)]


class FrameDepthPass(C.Structure):
    """ur_frame_depth_pass (include/ur_frame.h): the draws, target, optional counters and ur_depth_prepass flags of UR_FRAME_DEPTH_PASS."""
    _fields_ = [("draws", RasterDraws), ("depth", C.c_void_p), ("stats6", C.c_void_p), ("flags", C.c_uint32)]


class GBufferTargets(C.Structure):
    """ur_gbuffer_targets (include/ur_raster.h): the band's render targets, the optional ObjectId image and the key scratch of ur_gbuffer_pass."""
    _fields_ = [("gbuf_a", C.c_void_p), ("gbuf_b", C.c_void_p), ("gbuf_c", C.c_void_p), ("hdr", C.c_void_p), ("object_id", C.c_void_p),
                ("keys", C.c_void_p)]


class Texture2D(C.Structure):
    """ur_texture2d (include/ur_raster.h): `mips` tightly packed levels of R8G8B8A8 texels from the device address `texels`."""
    _fields_ = [("texels", C.c_uint64), ("width", C.c_uint16), ("height", C.c_uint16), ("mips", C.c_uint8), ("format", C.c_uint8), ("reserved", C.c_uint16)]


class Material(C.Structure):
    """ur_material (include/ur_raster.h): the textures t0-t3 and the pipeline key of one command slot, 80 bytes."""
    _fields_ = [("base_color", Texture2D), ("metallic_roughness", Texture2D), ("normal", Texture2D), ("emissive", Texture2D),
                ("pipeline_key", C.c_uint32), ("reserved", C.c_uint32 * 3)]


UR_TEXTURE_R8G8B8A8_UNORM = 28
UR_TEXTURE_R8G8B8A8_UNORM_SRGB = 29
UR_TEXTURE_BC1_UNORM, UR_TEXTURE_BC1_UNORM_SRGB, UR_TEXTURE_BC3_UNORM, UR_TEXTURE_BC3_UNORM_SRGB, UR_TEXTURE_BC5_UNORM = 71, 72, 77, 78, 83
# sources of ur_texture_transcode only, never Texture2D.format values
UR_TEXTURE_SOURCE_BC2_UNORM, UR_TEXTURE_SOURCE_BC2_UNORM_SRGB, UR_TEXTURE_SOURCE_BC4_UNORM = 74, 75, 80
UR_TEXTURE_SOURCE_BC7_UNORM, UR_TEXTURE_SOURCE_BC7_UNORM_SRGB = 98, 99
UR_MATERIAL_NORMAL_MAP, UR_MATERIAL_METALLIC_ROUGHNESS_MAP, UR_MATERIAL_BASE_COLOR_MAP, UR_MATERIAL_EMISSIVE_MAP = 1, 2, 4, 8
UR_MATERIAL_ALPHA_MASK = 0x10


class GBufferMask(C.Structure):
    """ur_gbuffer_mask (include/ur_raster.h): the alpha-masked selection of ur_gbuffer_pass_masked, its 64-bit scratch and optional counters."""
    _fields_ = [("draws", C.POINTER(RasterDraws)), ("keys64", C.c_void_p), ("stats6", C.c_void_p), ("won", C.c_void_p)]


class ForwardTargets(C.Structure):
    """ur_forward_targets (include/ur_raster.h): the band's HDR image and the key scratch of ur_forward_pass."""
    _fields_ = [("hdr", C.c_void_p), ("keys", C.c_void_p)]


class PickResult(C.Structure):
    """ur_pick_result (include/ur_raster.h): what ur_object_id_pick answers for one point, 16 bytes."""
    _fields_ = [("object_id", C.c_uint32), ("key", C.c_uint32), ("slot", C.c_uint32), ("depth_bits", C.c_uint32)]


UR_PICK_MAX_POINTS = 64


class FrameGBufferPass(C.Structure):
    """ur_frame_gbuffer_pass (include/ur_frame.h): the draws, targets, optional counters, ur_gbuffer_pass flags and key bits of UR_FRAME_GBUFFER_PASS."""
    _fields_ = [("draws", RasterDraws), ("targets", GBufferTargets), ("stats6", C.c_void_p), ("flags", C.c_uint32), ("key_triangle_bits", C.c_uint32)]


UR_RASTER_MAX_TARGET = 16384
UR_RASTER_INDEX_FORMAT_R32_UINT = 42
UR_DEPTH_QUANTIZE_D24 = 0x1
UR_DEPTH_GUARD_BAND = 2097152
UR_GBUFFER_PART_RASTER, UR_GBUFFER_PART_RESOLVE = 0x1, 0x2


class HzbSlice(C.Structure):
    """ur_hzb_slice: one contiguous run of floats of the HZB allocation."""
    _fields_ = [("offset", C.c_uint32), ("count", C.c_uint32)]


class SceneConstants(C.Structure):
    """FSceneConstants (Source/Render/RendererUtils.h:41-79)."""
    _fields_ = [
        ("World", C.c_float * 16), ("View", C.c_float * 16), ("ViewInverse", C.c_float * 16), ("Projection", C.c_float * 16),
        ("BaseColor", C.c_float * 3), ("LightIntensity", C.c_float),
        ("LightDirection", C.c_float * 3), ("Padding1", C.c_float),
        ("CameraPosition", C.c_float * 3), ("Padding2", C.c_float),
        ("LightColor", C.c_float * 3), ("Padding3", C.c_float),
        ("EmissiveFactor", C.c_float * 3), ("Padding4", C.c_float),
        ("LightViewProjection", C.c_float * 16),
        ("ShadowStrength", C.c_float), ("ShadowBias", C.c_float), ("ShadowMapSize", C.c_float * 2),
        ("MetallicFactor", C.c_float), ("RoughnessFactor", C.c_float), ("BaseColorAlpha", C.c_float), ("AlphaCutoff", C.c_float),
        ("AlphaMode", C.c_uint32), ("PaddingMaterial", C.c_uint32 * 3),
        ("BaseColorTransformOffsetScale", C.c_float * 4), ("BaseColorTransformRotation", C.c_float * 4),
        ("MetallicRoughnessTransformOffsetScale", C.c_float * 4), ("MetallicRoughnessTransformRotation", C.c_float * 4),
        ("NormalTransformOffsetScale", C.c_float * 4), ("NormalTransformRotation", C.c_float * 4),
        ("EmissiveTransformOffsetScale", C.c_float * 4), ("EmissiveTransformRotation", C.c_float * 4),
        ("EnvMapMipCount", C.c_float), ("PaddingEnvMap", C.c_float * 3),
        ("ObjectId", C.c_uint32), ("PaddingObjectId", C.c_float * 3),
    ]


class SkyConstants(C.Structure):
    """FSkyAtmosphereConstants (Source/Render/RendererUtils.h:81-92)."""
    _fields_ = [
        ("World", C.c_float * 16), ("View", C.c_float * 16), ("Projection", C.c_float * 16),
        ("CameraPosition", C.c_float * 3), ("Padding0", C.c_float),
        ("LightDirection", C.c_float * 3), ("Padding1", C.c_float),
        ("LightColor", C.c_float * 3), ("Padding2", C.c_float),
    ]


class LightingTables(C.Structure):
    _fields_ = [
        ("shadow_map", C.c_void_p), ("env_cube", C.c_void_p), ("env_base_size", C.c_uint32), ("env_mip_count", C.c_uint32),
        ("brdf_lut_rg16", C.c_void_p), ("lut_width", C.c_uint32), ("lut_height", C.c_uint32), ("env_cube_texels", C.c_uint64),
    ]


class MeshStream(C.Structure):
    """ur_mesh_stream (include/ur_mesh.h): one fp32 attribute stream of a glTF buffer."""
    _fields_ = [("offset", C.c_uint64), ("stride", C.c_uint32), ("present", C.c_uint32)]


class MeshPrimitive(C.Structure):
    """ur_mesh_primitive (include/ur_mesh.h), 112 bytes."""
    _fields_ = [("position", MeshStream), ("normal", MeshStream), ("texcoord", MeshStream), ("tangent", MeshStream), ("color", MeshStream),
                ("index_offset", C.c_uint64), ("index_count", C.c_uint32), ("index_component_type", C.c_uint32), ("mode", C.c_uint32),
                ("vertex_count", C.c_uint32), ("color_components", C.c_uint32), ("reserved", C.c_uint32)]


class MeshSection(C.Structure):
    """ur_mesh_section (include/ur_mesh.h)."""
    _fields_ = [("vertex_offset", C.c_uint32), ("index_start", C.c_uint32), ("index_count", C.c_uint32)]


class MeshLayout(C.Structure):
    """ur_mesh_layout (include/ur_mesh.h)."""
    _fields_ = [("vertex_count", C.c_uint32), ("index_count", C.c_uint32), ("scratch_bytes", C.c_uint64)]


class MeshInfo(C.Structure):
    """ur_mesh_info (include/ur_mesh.h), 56 bytes."""
    _fields_ = [("min", C.c_float * 3), ("max", C.c_float * 3), ("center", C.c_float * 3), ("radius", C.c_float), ("normals_regenerated", C.c_uint32),
                ("tangents_regenerated", C.c_uint32), ("skipped_determinant_triangles", C.c_uint32), ("out_of_range_triangles", C.c_uint32)]


UR_MESH_MODE_TRIANGLES, UR_MESH_MODE_TRIANGLE_STRIP, UR_MESH_MODE_TRIANGLE_FAN = 4, 5, 6
UR_MESH_INDEX_U8, UR_MESH_INDEX_U16, UR_MESH_INDEX_U32 = 5121, 5123, 5125
UR_MESH_BUILD_MAX_STREAM_OPS = 14


class SceneNode(C.Structure):
    """ur_scene_node (include/ur_scene_build.h), 144 bytes."""
    _fields_ = [("node_world", C.c_float * 16), ("scale", C.c_float * 3), ("max_scale", C.c_float), ("rotation", C.c_float * 9), ("translate", C.c_float * 3),
                ("reserved", C.c_uint32 * 4)]


class SceneMesh(C.Structure):
    """ur_scene_mesh (include/ur_scene_build.h), 32 bytes."""
    _fields_ = [("vertices", C.c_uint64), ("indices", C.c_uint64), ("vertex_bytes", C.c_uint32), ("index_bytes", C.c_uint32), ("stride", C.c_uint32),
                ("index_format", C.c_uint32)]


class SceneMaterialFactors(C.Structure):
    """ur_scene_material_factors (include/ur_scene_build.h), 176 bytes."""
    _fields_ = [("BaseColor", C.c_float * 3), ("BaseColorAlpha", C.c_float), ("EmissiveFactor", C.c_float * 3), ("MetallicFactor", C.c_float),
                ("RoughnessFactor", C.c_float), ("AlphaCutoff", C.c_float), ("AlphaMode", C.c_uint32), ("Padding", C.c_uint32), ("transforms", (C.c_float * 4) * 8)]


class SceneDraw(C.Structure):
    """ur_scene_draw (include/ur_scene_build.h), 32 bytes."""
    _fields_ = [(n, C.c_uint32) for n in ("node", "mesh", "material", "constants_slot", "object_id", "index_start", "index_count", "reserved")]


class SceneBuildSummary(C.Structure):
    """ur_scene_build_summary (include/ur_scene_build.h), 48 bytes."""
    _fields_ = [("scene_min", C.c_float * 3), ("scene_max", C.c_float * 3), ("scene_center", C.c_float * 3), ("scene_radius", C.c_float),
                ("draw_count", C.c_uint32), ("skipped_draws", C.c_uint32)]


class SceneBuildTables(C.Structure):
    """ur_scene_build_tables (include/ur_scene_build.h): the addresses and counts of the five tables."""
    _fields_ = [("nodes", C.c_void_p), ("meshes", C.c_void_p), ("mesh_infos", C.c_void_p), ("materials", C.c_void_p), ("draws", C.c_void_p),
                ("node_count", C.c_uint32), ("mesh_count", C.c_uint32), ("material_count", C.c_uint32), ("draw_count", C.c_uint32)]


class SceneBuildOutputs(C.Structure):
    """ur_scene_build_outputs (include/ur_scene_build.h): the addresses of the five outputs, the constants stride and the slot count."""
    _fields_ = [("bounds", C.c_void_p), ("commands", C.c_void_p), ("constants", C.c_void_p), ("centers", C.c_void_p), ("summary", C.c_void_p),
                ("constants_stride", C.c_uint32), ("slot_count", C.c_uint32)]


UR_SCENE_BUILD_MAX_STREAM_OPS = 3
UR_SCENE_BUILD_TRANSFORMS_ONLY = 0x1
UR_SCENE_BUILD_MAX_DRAWS = 1 << 24
# ur_env_cube.h
UR_ENV_SOURCE_RGBA16F, UR_ENV_SOURCE_BC6H_UF16, UR_ENV_SOURCE_BC6H_SF16 = 10, 95, 96
UR_ENV_CUBE_BUILD_MAX_STREAM_OPS = 3
UR_ENV_CUBE_MAX_BASE_SIZE = 16384
# ur_env_prefilter.h
UR_ENV_PREFILTER_MAX_BASE_SIZE, UR_ENV_PREFILTER_MIN_SAMPLES, UR_ENV_PREFILTER_MAX_SAMPLES = 2048, 16, 4096
UR_ENV_PREFILTER_MAX_STREAM_OPS = 15
# ur_env_panorama.h
UR_ENV_PANORAMA_MAX_WIDTH, UR_ENV_PANORAMA_MAX_HEIGHT, UR_ENV_PANORAMA_MAX_BASE_SIZE, UR_ENV_PANORAMA_MAX_TAPS = 16384, 8192, 2048, 16
UR_ENV_PANORAMA_MAX_STREAM_OPS = 1
# ur_env_sky.h
UR_ENV_SKY_MAX_BASE_SIZE, UR_ENV_SKY_MAX_TAPS, UR_ENV_SKY_MAX_STREAM_OPS = 2048, 16, 1
# ur_brdf_lut.h
UR_BRDF_LUT_MAX_WIDTH, UR_BRDF_LUT_MAX_HEIGHT, UR_BRDF_LUT_MIN_SAMPLES, UR_BRDF_LUT_MAX_SAMPLES = 1024, 256, 16, 4096
UR_BRDF_LUT_MAX_STREAM_OPS = 1


class DdsInfo(C.Structure):
    """ur_dds_info (include/ur_assets.h)."""
    _fields_ = [(n, C.c_uint32) for n in ("width", "height", "mip_count", "slices", "is_cube", "dxgi_format", "header_size", "block_dim", "bytes_per_block")]


class HdrInfo(C.Structure):
    """ur_hdr_info (include/ur_assets.h)."""
    _fields_ = [(n, C.c_uint32) for n in ("width", "height", "payload_offset", "rle")]


class SceneModel(C.Structure):
    """ur_scene_model (include/ur_scene.h)."""
    _fields_ = [("bounds_min", C.c_float * 3), ("bounds_max", C.c_float * 3), ("center", C.c_float * 3), ("radius", C.c_float),
                ("pipeline_key", C.c_uint32), ("material_index", C.c_uint32), ("model_index", C.c_uint32), ("node_order", C.c_uint32),
                ("mesh_index", C.c_uint32), ("primitive_index", C.c_uint32)]


class SceneSummary(C.Structure):
    _fields_ = [("model_count", C.c_uint32), ("scene_center", C.c_float * 3), ("scene_radius", C.c_float)]


class ScenePlanDraw(C.Structure):
    """ur_scene_plan_draw (include/ur_scene.h)."""
    _fields_ = [(n, C.c_uint32) for n in ("node", "mesh", "primitive", "material_index", "pipeline_key", "model_index", "constants_slot", "object_id")]


class TonemapConstants(C.Structure):
    """TonemapParams (Shaders/Tonemap.hlsl:22-28)."""
    _fields_ = [("EnableTonemap", C.c_uint32), ("EnableAutoExposure", C.c_uint32), ("Exposure", C.c_float), ("Gamma", C.c_float)]


class AutoExposureConstants(C.Structure):
    """AutoExposureConstants (Shaders/AutoExposure.hlsl:1-12), 36 bytes."""
    _fields_ = [("InputSize", C.c_float * 2), ("DeltaTime", C.c_float), ("AdaptationSpeedUp", C.c_float), ("AdaptationSpeedDown", C.c_float),
                ("UseHistory", C.c_uint32), ("AutoExposureKey", C.c_float), ("AutoExposureMin", C.c_float), ("AutoExposureMax", C.c_float)]


class CasConstants(C.Structure):
    """CasParams (Shaders/Cas.hlsl:44-49), 16 bytes."""
    _fields_ = [("TexelDelta", C.c_float * 2), ("Sharpness", C.c_float), ("Padding", C.c_float)]


class FramePost(C.Structure):
    """ur_frame_post (include/ur_frame.h): post-chain resources and parameters of a frame (ur_frame_set_post)."""
    _fields_ = [("luminance", C.c_void_p * 2), ("tonemap_scratch", C.c_void_p), ("delta_time", C.c_float),
                ("tonemap_exposure", C.c_float), ("tonemap_gamma", C.c_float),
                ("ae_key", C.c_float), ("ae_min", C.c_float), ("ae_max", C.c_float), ("ae_speed_up", C.c_float), ("ae_speed_down", C.c_float),
                ("cas_sharpness", C.c_float)]


class FrameTaa(C.Structure):
    """ur_frame_taa (include/ur_frame.h): the TemporalAA history ring of a frame (ur_frame_set_taa)."""
    _fields_ = [("history", C.POINTER(C.c_void_p)), ("history_count", C.c_uint32), ("history_weight", C.c_float)]


class FrameTaaInfo(C.Structure):
    """ur_frame_taa_info (include/ur_frame.h): what the next frame with UR_FRAME_TAA does (ur_frame_taa_next)."""
    _fields_ = [("read_slot", C.c_uint32), ("write_slot", C.c_uint32), ("use_history", C.c_uint32), ("jitter", C.c_float * 2)]


class DebugGlyph(C.Structure):
    """ur_debug_glyph (include/ur_hotpath.h) == FDebugPrintGlyph (Source/Render/DebugPrintFont.h:11-19), 40 bytes."""
    _fields_ = [("UvMin", C.c_float * 2), ("UvMax", C.c_float * 2), ("Size", C.c_float * 2), ("Offset", C.c_float * 2),
                ("Advance", C.c_float), ("Padding", C.c_float)]


class DebugPrintConstants(C.Structure):
    """ur_debug_print_constants == DebugPrintConstants (Shaders/GpuDebugPrint.hlsl:4-9)."""
    _fields_ = [("ScreenSize", C.c_float * 2), ("FirstChar", C.c_uint32), ("CharCount", C.c_uint32)]


class FrameDebugPrint(C.Structure):
    """ur_frame_debug_print (include/ur_frame.h): the text buffer and font of UR_FRAME_DEBUG_PRINT (ur_frame_set_debug_print)."""
    _fields_ = [("buffer", C.c_void_p), ("glyphs", C.c_void_p), ("glyph_count", C.c_uint32), ("atlas", C.c_void_p),
                ("atlas_w", C.c_uint32), ("atlas_h", C.c_uint32), ("first_char", C.c_uint32), ("char_count", C.c_uint32)]


UR_DEBUG_PRINT_MAX_ENTRIES = 4096


class FrameResources(C.Structure):
    """ur_frame_resources (include/ur_frame.h)."""
    _fields_ = [
        ("width", C.c_uint32), ("height", C.c_uint32), ("row0", C.c_uint32), ("rows", C.c_uint32),
        ("gbuffer_a", C.c_void_p), ("gbuffer_b", C.c_void_p), ("gbuffer_c", C.c_void_p), ("depth_band", C.c_void_p),
        ("lighting_band", C.c_void_p), ("depth_full", C.c_void_p), ("hzb", C.c_void_p),
        ("hzb_mips", MipDesc * UR_MAX_HZB_MIPS), ("hzb_mip_count", C.c_uint32),
        ("tables", LightingTables),
        ("model_bounds", C.c_void_p), ("indirect_args", C.c_void_p), ("indirect_command_count", C.c_uint32),
        ("instance_index_base", C.c_uint32), ("visible_indices", C.c_void_p), ("visible_count", C.c_void_p), ("cull_stats", C.c_void_p),
        ("tonemap_band", C.c_void_p),
    ]


UR_FRAME_INDIRECT_DRAW, UR_FRAME_HZB, UR_FRAME_DEPTH_PREPASS, UR_FRAME_SHADOWS, UR_FRAME_SKY = 0x1, 0x2, 0x4, 0x8, 0x10
UR_FRAME_FUSE_LIGHTING_SKY, UR_FRAME_GPU_TIMING, UR_FRAME_GRAPH_DUMP, UR_FRAME_BARRIER_LOGS = 0x20, 0x40, 0x80, 0x100
UR_FRAME_ASYNC_COMPUTE, UR_FRAME_ASYNC_NO_JOIN, UR_FRAME_TONEMAP, UR_FRAME_TIME_LIGHTING = 0x200, 0x400, 0x800, 0x1000
UR_FRAME_HZB_TAIL_WITH_LIGHTING = 0x2000
UR_FRAME_HZB_WITH_LIGHTING = 0x4000
UR_FRAME_TIME_LIGHTING_RECORD_COST = 0x8000
UR_FRAME_TIME_LIGHTING_KERNEL = 0x10000
UR_FRAME_HZB_SHARD = 0x20000
UR_FRAME_AUTO_EXPOSURE = 0x40000
UR_FRAME_CAS = 0x80000
UR_FRAME_FUSE_TONEMAP_CAS = 0x100000
UR_FRAME_POST_EXCHANGE = 0x200000
UR_FRAME_CULL_VIEWS = 0x400000
UR_FRAME_TAA = 0x800000
UR_FRAME_FUSE_TAA_TONEMAP = 0x1000000
UR_FRAME_TAA_BAND = 0x2000000
UR_FRAME_DEBUG_PRINT = 0x4000000
UR_FRAME_SHADOW_PASS = 0x8000000
UR_FRAME_DEPTH_PASS = 0x10000000
UR_FRAME_GBUFFER_PASS = 0x20000000
UR_FRAME_DEFAULT = UR_FRAME_INDIRECT_DRAW | UR_FRAME_HZB | UR_FRAME_DEPTH_PREPASS | UR_FRAME_SHADOWS | UR_FRAME_SKY

assert C.sizeof(SceneConstants) == 608 and C.sizeof(SkyConstants) == 240
assert C.sizeof(AutoExposureConstants) == 36 and C.sizeof(CasConstants) == 16
assert C.sizeof(DebugGlyph) == 40 and C.sizeof(DebugPrintConstants) == 16

# name -> (restype, argtypes); every symbol declared in include/*.h
_VP, _U32, _F = C.c_void_p, C.c_uint32, C.c_float
_FP = C.POINTER(C.c_float)
SIGNATURES = {
    # ur_hotpath.h
    "ur_create": (_VP, [C.c_int, _VP]),
    "ur_destroy": (None, [_VP]),
    "ur_reserve": (C.c_int, [_VP, _U32]),
    "ur_defer_hzb_tail": (C.c_int, [_VP, C.c_int]),
    "ur_flush": (C.c_int, [_VP]),
    "ur_debug_set_hzb_timeout": (C.c_int, [_VP]),
    "ur_debug_lighting_schedule": (C.c_int, [_VP, C.POINTER(_U32)]),
    "ur_debug_stream_ceiling": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, C.c_uint64, _VP, _VP]),
    "ur_debug_timeline": (C.c_int, [_VP, _VP, _U32]),
    "ur_time_next_lighting": (C.c_int, [_VP, _VP, _VP]),
    "ur_time_next_cull": (C.c_int, [_VP, _VP]),
    "ur_time_cull_carried": (C.c_int, [_VP]),
    "ur_set_option": (C.c_int, [_VP, C.c_int, C.c_int]),
    "ur_get_option": (C.c_int, [_VP, C.c_int, C.POINTER(C.c_int)]),
    "ur_last_error": (C.c_char_p, []),
    "ur_version": (C.c_char_p, []),
    "ur_hzb_layout": (_U32, [_U32, _U32, C.POINTER(MipDesc), C.POINTER(_U32)]),
    "ur_build_hzb": (C.c_int, [_VP, _VP, _U32, _U32, _VP, C.POINTER(MipDesc), _U32]),
    "ur_hzb_band_pieces": (C.c_int, [_U32, _U32, _U32, C.POINTER(_U32), C.POINTER(_U32)]),
    "ur_hzb_band_slices": (C.c_int, [C.POINTER(MipDesc), _U32, _U32, _U32, C.POINTER(HzbSlice)]),
    "ur_build_hzb_band": (C.c_int, [_VP, _VP, _U32, _U32, _VP, C.POINTER(MipDesc), _U32, _U32, _U32]),
    "ur_build_hzb_tail": (C.c_int, [_VP, _VP, C.POINTER(MipDesc), _U32]),
    "ur_cull_indirect_args": (C.c_int, [_VP, C.POINTER(_U32), _VP, _VP, C.POINTER(MipDesc), _VP, _VP, _VP, _VP]),
    "ur_cull_indirect_args_ex": (C.c_int, [_VP, C.POINTER(_U32), _VP, _VP, C.POINTER(MipDesc), _VP, _VP, _VP, _VP, _U32]),
    "ur_cull_indirect_args_draws": (C.c_int, [_VP, C.POINTER(_U32), _VP, _VP, C.POINTER(MipDesc), _VP, _VP, _VP, _VP, _U32,
                                              C.POINTER(DrawRanges)]),
    "ur_cull_indirect_args_views": (C.c_int, [_VP, C.POINTER(_U32), _VP, _VP, C.POINTER(MipDesc), _VP, _VP, _VP, _VP, _U32,
                                              C.POINTER(DrawRanges), C.POINTER(CullView), _U32]),
    "ur_env_cube_texels": (C.c_size_t, [_U32, _U32]),
    "ur_stage_env_cube": (C.c_int, [_VP, _VP, _U32, _U32, _VP]),
    "ur_deferred_lighting": (C.c_int, [_VP, C.POINTER(SceneConstants), _VP, _VP, _VP, C.POINTER(LightingTables), _VP, _U32, _U32, _U32, _U32]),
    "ur_sky_atmosphere": (C.c_int, [_VP, C.POINTER(SkyConstants), _VP, _VP, _U32, _U32, _U32, _U32]),
    "ur_deferred_lighting_sky": (C.c_int, [_VP, C.POINTER(SceneConstants), C.POINTER(SkyConstants), _VP, _VP, _VP, _VP,
                                           C.POINTER(LightingTables), _VP, _U32, _U32, _U32, _U32]),
    "ur_tonemap": (C.c_int, [_VP, C.POINTER(TonemapConstants), _VP, _VP, _VP, _U32, _U32]),
    "ur_temporal_aa": (C.c_int, [_VP, _VP, _VP, _VP, _F, _U32, _U32, _U32, _U32, _U32]),
    "ur_temporal_aa_tonemap": (C.c_int, [_VP, C.POINTER(TonemapConstants), _VP, _VP, _VP, _VP, _VP, _F, _U32, _U32, _U32, _U32, _U32]),
    "ur_auto_exposure": (C.c_int, [_VP, C.POINTER(AutoExposureConstants), _VP, _U32, _U32, _VP, _VP]),
    "ur_cas": (C.c_int, [_VP, C.POINTER(CasConstants), _VP, _VP, _U32, _U32, _U32, _U32]),
    "ur_tonemap_cas": (C.c_int, [_VP, C.POINTER(TonemapConstants), C.POINTER(CasConstants), _VP, _VP, _VP, _U32, _U32, _U32, _U32]),
    "ur_post_record_bytes": (C.c_uint64, [_U32]),
    "ur_pack_post_record": (C.c_int, [_VP, _VP, _U32, _U32, _U32, _U32, _VP]),
    "ur_auto_exposure_records": (C.c_int, [_VP, C.POINTER(AutoExposureConstants), _VP, _U32, _U32, _U32, _VP, _VP]),
    "ur_tonemap_cas_halo": (C.c_int, [_VP, C.POINTER(TonemapConstants), C.POINTER(CasConstants), _VP, _VP, _VP, _VP, _VP, _U32, _U32, _U32, _U32]),
    "ur_cas_halo": (C.c_int, [_VP, C.POINTER(TonemapConstants), C.POINTER(CasConstants), _VP, _VP, _VP, _VP, _VP, _U32, _U32, _U32, _U32]),
    "ur_taa_record_bytes": (C.c_uint64, [_U32]),
    "ur_pack_taa_record": (C.c_int, [_VP, _VP, _VP, _U32, _U32, _U32, _U32, _U32, _VP]),
    "ur_temporal_aa_halo": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _F, _U32, _U32, _U32, _U32, _U32]),
    "ur_temporal_aa_tonemap_halo": (C.c_int, [_VP, C.POINTER(TonemapConstants), _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _F,
                                              _U32, _U32, _U32, _U32, _U32]),
    "ur_debug_print_buffer_bytes": (C.c_uint64, []),
    "ur_debug_print_reset": (C.c_int, [_VP, _VP, _VP]),
    "ur_debug_print_stats": (C.c_int, [_VP, _VP, _VP]),
    "ur_debug_print_text": (C.c_int, [_VP, _VP, _U32, _U32, _U32, C.c_char_p, _U32]),
    "ur_debug_print_draw": (C.c_int, [_VP, C.POINTER(DebugPrintConstants), _VP, _U32, _VP, _U32, _U32, _VP, _VP, _U32, _U32, _U32, _U32]),
    "ur_allgather_rows": (C.c_int, [_VP, _VP, _VP, _U32, _U32, _U32, _U32]),
    "ur_allgather_rows_bytes": (C.c_int, [_VP, _VP, _VP, _U32, _U32, _U32, _U32]),
    "ur_allgather_rows_bytes_ex": (C.c_int, [_VP, _VP, _VP, _U32, _U32, _U32, _U32, C.c_int]),
    # ur_raster.h
    "ur_shadow_map": (C.c_int, [_VP, _FP, C.POINTER(RasterDraws), _VP, _U32, _U32, _VP]),
    "ur_raster_reserve": (C.c_int, [_VP, _U32]),
    "ur_depth_prepass": (C.c_int, [_VP, _FP, _FP, C.POINTER(RasterDraws), _VP, _U32, _U32, _U32, _VP]),
    "ur_gbuffer_pass": (C.c_int, [_VP, _FP, _FP, C.POINTER(RasterDraws), _VP, C.POINTER(GBufferTargets), _U32, _U32, _U32, _U32, _U32, _U32, _VP]),
    "ur_gbuffer_pass_parts": (C.c_int, [_VP, _FP, _FP, C.POINTER(RasterDraws), _VP, C.POINTER(GBufferTargets), _U32, _U32, _U32, _U32, _U32, _U32, _VP, _U32]),
    "ur_gbuffer_pass_materials": (C.c_int, [_VP, _FP, _FP, C.POINTER(RasterDraws), _VP, C.POINTER(GBufferTargets), _U32, _U32, _U32, _U32, _U32, _U32, _VP, _VP, _U32]),
    "ur_gbuffer_pass_masked": (C.c_int, [_VP, _FP, _FP, C.POINTER(RasterDraws), _VP, C.POINTER(GBufferTargets), _U32, _U32, _U32, _U32, _U32, _U32, _VP, _VP, _U32,
                                         C.POINTER(GBufferMask)]),
    "ur_gbuffer_pass_masked_parts": (C.c_int, [_VP, _FP, _FP, C.POINTER(RasterDraws), _VP, C.POINTER(GBufferTargets), _U32, _U32, _U32, _U32, _U32, _U32, _VP, _U32,
                                               _VP, _U32, C.POINTER(GBufferMask)]),
    "ur_gbuffer_pass_materials_parts": (C.c_int, [_VP, _FP, _FP, C.POINTER(RasterDraws), _VP, C.POINTER(GBufferTargets), _U32, _U32, _U32, _U32, _U32, _U32, _VP, _U32,
                                                  _VP, _U32]),
    "ur_forward_pass": (C.c_int, [_VP, _FP, _FP, C.POINTER(RasterDraws), _VP, C.POINTER(ForwardTargets), _U32, _U32, _U32, _U32, _U32, _U32, _VP, _VP, _U32,
                                  C.POINTER(GBufferMask), C.POINTER(SceneConstants), C.POINTER(LightingTables)]),
    "ur_forward_pass_parts": (C.c_int, [_VP, _FP, _FP, C.POINTER(RasterDraws), _VP, C.POINTER(ForwardTargets), _U32, _U32, _U32, _U32, _U32, _U32, _VP, _U32,
                                        _VP, _U32, C.POINTER(GBufferMask), C.POINTER(SceneConstants), C.POINTER(LightingTables)]),
    "ur_object_id_pass": (C.c_int, [_VP, _FP, _FP, C.POINTER(RasterDraws), _VP, _VP, _VP, _U32, _U32, _U32, _U32, _U32, _U32, _VP]),
    "ur_object_id_pick": (C.c_int, [_VP, _FP, _FP, C.POINTER(RasterDraws), _VP, _U32, _U32, _U32, _U32, C.POINTER(_U32), _U32, _VP, _VP]),
    "ur_texture_transcode_bytes": (C.c_uint64, [_U32, _U32, _U32]),
    "ur_texture_transcode": (C.c_int, [_VP, _U32, _VP, _U32, _U32, _U32, _VP, C.POINTER(Texture2D)]),
    # ur_mesh.h
    "ur_mesh_layout_of": (C.c_int, [C.POINTER(MeshPrimitive), _U32, C.c_uint64, C.POINTER(MeshLayout), C.POINTER(MeshSection)]),
    "ur_mesh_build": (C.c_int, [_VP, _VP, C.c_uint64, C.POINTER(MeshPrimitive), _U32, _VP, _VP, _VP, C.c_uint64, _VP]),
    # ur_scene_build.h
    "ur_scene_build_scratch_bytes": (C.c_uint64, [_U32]),
    "ur_scene_build": (C.c_int, [_VP, C.POINTER(SceneBuildTables), C.POINTER(SceneConstants), C.POINTER(SceneBuildOutputs), _VP, C.c_uint64, _U32]),
    # ur_env_cube.h
    "ur_env_cube_source_bytes": (C.c_size_t, [_U32, _U32, _U32]),
    "ur_env_cube_build": (C.c_int, [_VP, _VP, C.c_size_t, _U32, _U32, _U32, _VP, C.c_size_t, _VP]),
    # ur_env_prefilter.h
    "ur_env_prefilter_table_bytes": (C.c_size_t, [_U32, _U32]),
    "ur_env_prefilter_scratch_bytes": (C.c_size_t, [_U32]),
    "ur_env_prefilter": (C.c_int, [_VP, _VP, C.c_size_t, _U32, _U32, _VP, C.c_size_t, _VP, C.c_size_t, _VP, C.c_size_t]),
    # ur_env_panorama.h
    "ur_env_panorama": (C.c_int, [_VP, _VP, C.c_size_t, _U32, _U32, _U32, _U32, _VP, C.c_size_t]),
    # ur_env_sky.h
    "ur_env_sky": (C.c_int, [_VP, C.POINTER(SkyConstants), _U32, _U32, _VP, C.c_size_t]),
    # ur_brdf_lut.h
    "ur_brdf_lut_table_bytes": (C.c_size_t, [_U32, _U32]),
    "ur_brdf_lut": (C.c_int, [_VP, _U32, _U32, _U32, _VP, C.c_size_t, _VP, C.c_size_t]),
    # ur_assets.h
    "ur_hdr_parse": (C.c_int, [_VP, C.c_size_t, C.POINTER(HdrInfo)]),
    "ur_hdr_unpack": (C.c_int, [_VP, C.c_size_t, C.POINTER(HdrInfo), _VP]),
    "ur_hdr_last_error": (C.c_char_p, []),
    "ur_dds_parse":(C.c_int, [_VP, C.c_size_t, C.POINTER(DdsInfo)]),
    "ur_dds_parse_texture2d": (C.c_int, [_VP, C.c_size_t, C.POINTER(DdsInfo)]),
    "ur_dds_parse_texture2d_source": (C.c_int, [_VP, C.c_size_t, C.POINTER(DdsInfo)]),
    "ur_dds_texel_count": (C.c_size_t, [C.POINTER(DdsInfo)]),
    "ur_dds_decode_rgba16f": (C.c_int, [_VP, C.c_size_t, C.POINTER(DdsInfo), _VP, C.POINTER(_U32)]),
    "ur_dds_copy_rg16": (C.c_int, [_VP, C.c_size_t, C.POINTER(DdsInfo), _VP]),
    "ur_bc6h_decode_block": (C.c_int, [_VP, C.c_int, _VP]),
    "ur_bc6h_block_endpoints": (C.c_int, [_VP, C.c_int, _VP]),
    # ur_scene.h
    "ur_scene_model_count": (C.c_int, [C.c_char_p]),
    "ur_scene_model_path": (C.c_int, [C.c_char_p, _U32, C.c_char_p, _U32]),
    "ur_scene_extract": (C.c_int, [C.c_char_p, C.POINTER(C.c_char_p), _U32, C.POINTER(SceneModel), _U32, C.POINTER(SceneSummary)]),
    "ur_scene_plan": (C.c_int, [C.c_char_p, C.POINTER(C.c_char_p), _U32, C.POINTER(_U32), C.POINTER(SceneNode), _U32, C.POINTER(_U32),
                                C.POINTER(ScenePlanDraw), _U32, C.POINTER(_U32)]),
    # ur_frame.h
    "ur_frame_create": (_VP, [_VP, _VP, _U32, C.c_int, C.c_int]),
    "ur_frame_destroy": (None, [_VP]),
    "ur_frame_render": (C.c_int, [_VP, C.POINTER(FrameResources), C.POINTER(_U32), C.POINTER(SceneConstants), C.POINTER(SkyConstants), _U32]),
    "ur_frame_join_async": (None, [_VP]),
    "ur_frame_lighting_times": (_U32, [_VP, _FP, _U32]),
    "ur_frame_lighting_times_ex": (_U32, [_VP, _FP, _FP, _U32]),
    "ur_frame_hzb_ready": (C.c_int, [_VP]),
    "ur_frame_reset_hzb": (None, [_VP]),
    "ur_frame_set_post": (C.c_int, [_VP, C.POINTER(FramePost)]),
    "ur_frame_reset_post": (None, [_VP]),
    "ur_frame_set_taa": (C.c_int, [_VP, C.POINTER(FrameTaa)]),
    "ur_frame_reset_taa": (None, [_VP]),
    "ur_frame_taa_next": (C.c_int, [_VP, C.POINTER(FrameTaaInfo)]),
    "ur_frame_set_draw_ranges": (C.c_int, [_VP, C.POINTER(DrawRanges)]),
    "ur_frame_set_cull_views": (C.c_int, [_VP, C.POINTER(CullView), _U32]),
    "ur_frame_set_post_records": (C.c_int, [_VP, _VP, _VP]),
    "ur_frame_set_taa_records": (C.c_int, [_VP, _VP, _VP]),
    "ur_frame_finish_post": (C.c_int, [_VP]),
    "ur_frame_set_debug_print": (C.c_int, [_VP, C.POINTER(FrameDebugPrint)]),
    "ur_frame_set_shadow_pass": (C.c_int, [_VP, C.POINTER(FrameShadowPass)]),
    "ur_frame_set_depth_pass": (C.c_int, [_VP, C.POINTER(FrameDepthPass)]),
    "ur_frame_set_gbuffer_pass": (C.c_int, [_VP, C.POINTER(FrameGBufferPass)]),
    "ur_frame_set_gbuffer_materials": (C.c_int, [_VP, _VP, _U32]),
    "ur_frame_report": (_U32, [_VP, C.c_char_p, _U32]),
    "ur_rg_timing_stats": (_U32, [C.c_char_p, _U32]),
    # ur_host.h
    "ur_host_look_to_lh": (None, [_FP, _FP, _FP, _FP]),
    "ur_host_look_at_lh": (None, [_FP, _FP, _FP, _FP]),
    "ur_host_reverse_z_projection": (None, [_F, _F, _F, _FP]),
    "ur_host_orthographic_lh": (None, [_F, _F, _F, _F, _FP]),
    "ur_host_mat_mul": (None, [_FP, _FP, _FP]),
    "ur_host_mat_inverse": (C.c_int, [_FP, _FP]),
    "ur_host_frustum_planes": (None, [_FP, _FP]),
    "ur_host_is_aabb_in_frustum": (C.c_int, [_FP, _FP, _FP]),
    "ur_host_light_view_projection": (None, [_FP, _F, _FP, _FP]),
    "ur_host_pack_culling_constants": (None, [_FP, _FP, _U32, _U32, _U32, _U32, _U32, _U32, C.POINTER(_U32)]),
    "ur_host_fill_scene_constants": (None, [_FP, _FP, _FP, _F, _FP, _FP, _FP, _F, _F, _F, _F, _F, C.POINTER(SceneConstants)]),
    "ur_host_fill_sky_constants": (None, [_FP, _FP, _FP, _F, _FP, _FP, C.POINTER(SkyConstants)]),
    "ur_host_taa_jitter": (None, [_U32, _FP]),
    "ur_host_apply_taa_jitter": (None, [_FP, _FP, _F, _F]),
    "ur_host_srgb_encode_table": (None, [_FP]),
    "ur_host_srgb_decode_table": (None, [_FP]),
    "ur_host_lod_table": (None, [_FP]),
    "ur_host_bc_chain_bytes": (C.c_uint64, [_U32, _U32, _U32, _U32]),
    "ur_host_bc_decode_level": (C.c_int, [_U32, _VP, _U32, _U32, _VP]),
    "ur_host_texture_chain_bytes": (C.c_uint64, [_U32, _U32, _U32, _U32]),
    "ur_host_texture_decode_level": (C.c_int, [_U32, _VP, _U32, _U32, _VP]),
    "ur_host_mesh_build": (C.c_int, [_VP, C.c_uint64, C.POINTER(MeshPrimitive), _U32, _VP, _VP, C.POINTER(MeshSection), C.POINTER(MeshInfo)]),
    "ur_host_scene_build": (C.c_int, [C.POINTER(SceneBuildTables), C.POINTER(SceneConstants), C.POINTER(SceneBuildOutputs), C.c_uint64, _U32]),
    "ur_host_env_cube_build": (C.c_int, [_VP, C.c_size_t, _U32, _U32, _U32, _VP, C.c_size_t, _VP]),
    "ur_host_env_prefilter_table": (C.c_int, [_U32, _U32, _VP, C.c_size_t]),
    "ur_host_env_prefilter": (C.c_int, [_VP, C.c_size_t, _U32, _U32, _VP, C.c_size_t, _VP, C.c_size_t]),
    "ur_host_env_panorama_taps": (_U32, [_U32, _U32, _U32]),
    "ur_host_env_panorama": (C.c_int, [_VP, C.c_size_t, _U32, _U32, _U32, _U32, _VP, C.c_size_t]),
    "ur_host_env_sky_params": (C.c_int, [C.POINTER(SkyConstants), _FP]),
    "ur_host_env_sky": (C.c_int, [C.POINTER(SkyConstants), _U32, _U32, _VP, C.c_size_t]),
    "ur_host_brdf_lut_table": (C.c_int, [_U32, _U32, _VP, C.c_size_t]),
    "ur_host_brdf_lut": (C.c_int, [_U32, _U32, _U32, _VP, C.c_size_t, _VP, C.c_size_t]),
    "ur_host_debug_font": (C.c_int, [_VP, _U32, _VP, _U32, C.POINTER(_U32)]),
    "ur_host_direction_from_euler_degrees": (None, [_F, _F, _FP]),
    "ur_host_camera_forward_from_euler_degrees": (None, [_F, _F, _FP]),
    "ur_host_light_direction_roundtrip": (None, [_FP, _FP]),
}

_lib = None


def library_path() -> Path:
    return _LIB_PATH


def load() -> C.CDLL:
    """Load libur_hotpath.so; raise loudly if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not _LIB_PATH.exists():
        raise RuntimeError(
            f"{_LIB_PATH} is missing: the HIP extension is not built. Run `python -m unclerenderer_amd.build`. "
            "There is no CPU fallback for the hot path.")
    # One HIP runtime per process: torch bundles its own libamdhip64 (SONAME libamdhip64.so.7) but asks for it by file
    # name, so if the system copy were loaded first the process would end up with two runtimes and the second one sees
    # no device (KFD allows one open per process). Importing torch first makes our NEEDED libamdhip64.so.7 resolve to
    # the copy torch already loaded. A C++ host that does not use torch simply gets /opt/rocm's runtime.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(str(_LIB_PATH))
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if a declared symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


class UrError(RuntimeError):
    def __init__(self, code: int, where: str):
        msg = load().ur_last_error().decode(errors="replace")
        super().__init__(f"{where} failed with {code}: {msg}")
        self.code = code


def check(code: int, where: str) -> None:
    if code != UR_OK:
        raise UrError(code, where)


def fptr(a: np.ndarray):
    """float32 numpy array -> float* (the array must stay alive for the duration of the call)."""
    assert a.dtype == np.float32 and a.flags.c_contiguous
    return a.ctypes.data_as(_FP)
