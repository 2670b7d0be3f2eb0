/*
 * ur_host.h — host-side math of the callers of the hot path: the code that fills the constant blocks the four
 * passes receive. Plain fp32 C, no DirectXMath (the reference takes these from DirectXMath, which is outside the
 * repository: SURVEY.md §8c). Row-major matrices, row-vector convention.
 */
#ifndef UR_HOST_H
#define UR_HOST_H

#include <stdint.h>

#include "ur_brdf_lut.h"
#include "ur_env_cube.h"
#include "ur_env_panorama.h"
#include "ur_env_prefilter.h"
#include "ur_env_sky.h"
#include "ur_hotpath.h"
#include "ur_mesh.h"
#include "ur_scene_build.h"

#ifdef __cplusplus
extern "C" {
#endif

/* XMMatrixLookToLH as used by FCamera::GetViewMatrix (Source/Scene/Camera.cpp:23-31). */
void ur_host_look_to_lh(const float eye[3], const float dir[3], const float up[3], float out[16]);
/* XMMatrixLookAtLH (RendererUtils.cpp:1129). */
void ur_host_look_at_lh(const float eye[3], const float at[3], const float up[3], float out[16]);
/* Reverse-Z infinite projection, FCamera::GetProjectionMatrix (Source/Scene/Camera.cpp:33-47). */
void ur_host_reverse_z_projection(float fov_y, float aspect, float near_clip, float out[16]);
/* XMMatrixOrthographicLH (RendererUtils.cpp:1133). */
void ur_host_orthographic_lh(float w, float h, float zn, float zf, float out[16]);
void ur_host_mat_mul(const float a[16], const float b[16], float out[16]);
/* General 4x4 inverse (XMMatrixInverse); returns 0 when singular. */
int ur_host_mat_inverse(const float m[16], float out[16]);

/* BuildFrustumPlanesFromMatrix (RendererUtils.cpp:1151-1190): L, R, B, T, plane 4 = column 3 alone, plane 5 =
 * column 4 - column 3; each divided by |xyz| with no zero guard, so the reverse-Z infinite projection makes plane 4
 * (NaN,NaN,NaN,+inf) — kept, it never rejects. */
void ur_host_frustum_planes(const float view_proj[16], float planes[24]);
/* IsAabbInCameraFrustum (RendererUtils.cpp:1192-1218). */
int ur_host_is_aabb_in_frustum(const float planes[24], const float bmin[3], const float bmax[3]);
/* BuildDirectionalLightViewProjection (RendererUtils.cpp:1117-1137). */
void ur_host_light_view_projection(const float center[3], float radius, const float light_dir[3], float out[16]);

/* The 46 root constants of FRenderer::DispatchGpuCulling (Renderer.cpp:411-429). */
void ur_host_pack_culling_constants(const float view[16], const float proj[16], uint32_t model_count, uint32_t hzb_enabled,
                                    uint32_t hzb_mip_count, uint32_t hzb_width, uint32_t hzb_height, uint32_t debug_print,
                                    uint32_t out[UR_CULL_CONSTANT_DWORDS]);

/* RendererUtils::UpdateSceneConstants (RendererUtils.cpp:1029-1088) for the fields the lighting pass reads; the
 * material fields keep FSceneConstants' defaults (RendererUtils.h:41-79). */
void ur_host_fill_scene_constants(const float view[16], const float proj[16], const float camera_pos[3], float light_intensity,
                                  const float light_dir[3], const float light_color[3], const float light_view_proj[16],
                                  float shadow_strength, float shadow_bias, float shadow_w, float shadow_h, float env_mip_count,
                                  ur_scene_constants* out);
/* FDeferredRenderer::UpdateSkyConstants + RendererUtils::UpdateSkyConstants (DeferredRenderer.cpp:3789-3801,
 * RendererUtils.cpp:1090-1115): World = scale(radius) * translate(camera). */
void ur_host_fill_sky_constants(const float view[16], const float proj[16], const float camera_pos[3], float sky_radius,
                                const float light_dir[3], const float light_color[3], ur_sky_constants* out);

/* BuildTaaJitter (DeferredRenderer.cpp:47-67): (Halton(sample_index + 1, 2) - 0.5, Halton(sample_index + 1, 3) - 0.5) in fp32,
 * in pixels. The renderer's sample index runs 0..7 (ur_frame_taa_next). */
void ur_host_taa_jitter(uint32_t sample_index, float out[2]);
/* The jittered projection of a frame with history (DeferredRenderer.cpp:415-421): _31 += 2 jx / width, _32 += 2 jy / height
 * (elements 8 and 9); nothing when width or height is not positive. */
void ur_host_apply_taa_jitter(float proj[16], const float jitter[2], float width, float height);

/* The linear -> sRGB8 encode of the GBuffer resolve (ur_gbuffer_pass) as 255 ascending fp32 thresholds: the code of x
 * is the number of entries with x >= entry (a NaN gives 0). Entry c - 1, c = 1..255, is the linear value of sRGB (c - 0.5) / 255 by the
 * IEC 61966-2-1 curve, evaluated in double and rounded to fp32: the device reads these very bytes. */
void ur_host_srgb_encode_table(float out[255]);

/* The sRGB8 -> linear decode of a UR_TEXTURE_R8G8B8A8_UNORM_SRGB texel's R, G and B (ur_gbuffer_pass_materials): entry c,
 * c = 0..255, is the linear value of sRGB c / 255 by the IEC 61966-2-1 curve, evaluated in double and rounded to fp32: the device reads
 * these very bytes. */
void ur_host_srgb_decode_table(float out[256]);

/* The level-of-detail thresholds of the textured GBuffer resolve: entry j - 1, j = 1..127, is 2^(j / 128), evaluated in
 * double and rounded to fp32, ascending. With rho^2 = m * 2^e, m in [1, 2) from the float's bits, the 8.8 fixed-point level is
 * 128 e + (the number of entries with m >= entry) = floor(256 log2 rho): the device reads these very bytes. */
void ur_host_lod_table(float out[127]);

/* The block-compressed formats of the material sampler (UR_TEXTURE_BC*), on the host: these two run csrc/bc_decode.h,
 * the very functions the kernels decode with.
 * Bytes of a chain of `mips` levels of a width x height texture as ur_texture2d lays it out; 0 for a format that is not one of the five
 * BC codes, a zero dimension, a dimension above 65535, or mips outside 1..255. */
uint64_t ur_host_bc_chain_bytes(uint32_t format, uint32_t width, uint32_t height, uint32_t mips);
/* One level of ((level_width + 3) >> 2) x ((level_height + 3) >> 2) blocks, row-major -> level_width x level_height RGBA8 code words,
 * row-major, R in byte 0 (the _SRGB formats give the same codes as their UNORM twins: the decode to linear comes behind the code word).
 * UR_EINVAL for a null pointer, a format that is not one of the five BC codes or a zero dimension. */
int ur_host_bc_decode_level(uint32_t format, const void* blocks, uint32_t level_width, uint32_t level_height, uint8_t* rgba8_out);

/* The same two over the ten source formats of ur_texture_transcode (include/ur_raster.h): 71, 72, 77, 78, 83 and
 * UR_TEXTURE_SOURCE_* 74, 75, 80, 98, 99. They run csrc/bc_wide_decode.h, the very functions the transcode kernel decodes with.
 * Bytes of the source chain: 8 bytes a block for BC1 and BC4, 16 for the rest, in the layout above; 0 for any other format, a zero
 * dimension, a dimension above 65535, or mips outside 1..255. */
uint64_t ur_host_texture_chain_bytes(uint32_t format, uint32_t width, uint32_t height, uint32_t mips);
/* One level of blocks -> level_width x level_height RGBA8 code words, as ur_host_bc_decode_level. UR_EINVAL for a null pointer, a format
 * outside the ten or a zero dimension. */
int ur_host_texture_decode_level(uint32_t format, const void* blocks, uint32_t level_width, uint32_t level_height, uint8_t* rgba8_out);

/* ur_mesh_build (include/ur_mesh.h) on the host, serial, in the reference's order: the CPU fallback and the time baseline.
 * It runs csrc/mesh_rule.h, the very per-triangle and per-vertex functions the kernels run, and gives the device build's bytes. All
 * pointers are host memory; `buffer` may lie at any address. vertices_out takes 64 * V bytes, indices_out I words (ur_mesh_layout_of);
 * sections_out n entries, or NULL. UR_EINVAL for a null pointer and for everything ur_mesh_layout_of refuses. */
int ur_host_mesh_build(const void* buffer, uint64_t buffer_size, const ur_mesh_primitive* primitives, uint32_t n, void* vertices_out, uint32_t* indices_out,
                       ur_mesh_section* sections_out, ur_mesh_info* info_out);

/* ur_scene_build (include/ur_scene_build.h) on the host, serial, draw by draw in command order: the CPU fallback and the time
 * baseline. It runs csrc/scene_rule.h, the very functions the kernels run, and gives the device build's bytes. All pointers are host
 * memory at any alignment; no scratch. A command's ConstantBufferAddress is constants_address + slot * constants_stride: the caller
 * gives the address the records will have where the commands are read. UR_EINVAL for a null pointer (centers may be null),
 * draw_count == 0 or >= 2^24, an empty table, slot_count == 0, a stride below 608 or no multiple of 16, unknown flag bits. */
int ur_host_scene_build(const ur_scene_build_tables* tables, const ur_scene_constants* frame, const ur_scene_build_outputs* outputs,
                        uint64_t constants_address, uint32_t flags);

/* ur_env_cube_build (include/ur_env_cube.h) on the host, serial: the CPU fallback and the byte reference. It decodes with
 * csrc/bc6h_decode.h, the very functions the kernels decode with, and stages with the function ur_stage_env_cube runs; it gives the device
 * build's bytes, and in *reserved_blocks (or NULL) the device build's info word. All pointers are host memory; no GPU is needed. The same
 * refusals as ur_env_cube_build but for the context: UR_EINVAL for a null source or destination, an unknown format, a cube
 * ur_env_cube_texels refuses or a base size above UR_ENV_CUBE_MAX_BASE_SIZE, src_bytes or dst_texels that are not the cube's, a source or
 * destination that is not 16-byte aligned, and source, destination and reserved_blocks overlapping. */
int ur_host_env_cube_build(const void* src_host, size_t src_bytes, uint32_t format, uint32_t base_size, uint32_t mip_count, ur_half4* dst_host,
                           size_t dst_texels, uint32_t* reserved_blocks);

/* The sample table of the environment prefilter (include/ur_env_prefilter.h): for every level k = 1 .. L - 1 of a cube of
 * edge base_size, alpha = (k / (L - 1))^2, the sample_count Hammersley points' GGX half vectors give (with V = N) the tangent-space light
 * vector l = (2 hz hx, 2 hz hy, 2 hz^2 - 1) and the source level clamp(0.5 log2(Omega_s / Omega_p), 0, L - 1) with
 * Omega_s = 4 / (sample_count D(hz)), Omega_p = 4 pi / (6 base_size^2), all in double, each
 * rounded to fp32; samples with l.z <= 0 are dropped (sixteen zero bytes). L headers of 16 bytes come first: {fp32 1 / sum of the kept
 * l.z, uint32 samples kept, 0, 0}, level 0's {1, 0, 0, 0}; then 16 bytes a sample a level. The device reads these very bytes. Writes
 * ur_env_prefilter_table_bytes(base_size, sample_count) bytes; UR_EINVAL for a null out, numbers that function refuses or fewer out_bytes. */
int ur_host_env_prefilter_table(uint32_t base_size, uint32_t sample_count, void* out, size_t out_bytes);

/* ur_env_prefilter (include/ur_env_prefilter.h) on the host, serial: the CPU fallback and the byte reference, over csrc/env_prefilter_rule.h,
 * the very functions the kernels run - the pyramid, its bordered faces and the sums in the device's order. It allocates its own scratch.
 * All pointers are host memory; no GPU is needed. The same refusals as ur_env_prefilter but for the context and the scratch. */
int ur_host_env_prefilter(const void* src_host, size_t src_bytes, uint32_t base_size, uint32_t sample_count, const void* table_host, size_t table_bytes,
                          void* dst_host, size_t dst_bytes);

/* The taps a side ur_env_panorama (include/ur_env_panorama.h) is recommended to take for a width x height panorama and a
 * cube of edge base_size: the smallest power of two K with 3 K base_size >= 2 width and 3 K base_size >= 4 height, at most 16 - sub-samples
 * at most about half a panorama texel apart at a face's centre. 0 for sizes ur_env_panorama refuses. */
uint32_t ur_host_env_panorama_taps(uint32_t width, uint32_t height, uint32_t base_size);

/* ur_env_panorama on the host, serial: the CPU fallback and the byte reference, over csrc/env_panorama_rule.h, the very functions the
 * kernel runs, every texel's taps summed in the rule's 64-lane order. All pointers are host memory; no GPU is needed. The same refusals
 * as ur_env_panorama but for the context. */
int ur_host_env_panorama(const void* rgbe_host, size_t rgbe_bytes, uint32_t width, uint32_t height, uint32_t base_size, uint32_t taps, void* dst_host,
                         size_t dst_bytes);

/* The values ur_env_sky (include/ur_env_sky.h) folds the constants to, computed in double and each rounded once to fp32:
 * out[0..2] the normalised LightDirection; out[3..5] rayleighColor * exp(-h / 8000) * 3 / (16 * 3.14159265) with h = max(0,
 * CameraPosition[1]); out[6..8] LightColor * exp(-h / 1200) * 0.8 * (1 - 0.76^2) / (4 * 3.14159265); out[9] saturate(exp(-max(0, 1 - sun.y)
 * * 2)). The shader's literals are the fp32 values, widened exactly. The device build and ur_host_env_sky use these very floats. UR_EINVAL
 * for a null pointer, a CameraPosition[1], LightDirection or LightColor that is not finite, or a LightDirection of length zero. */
int ur_host_env_sky_params(const ur_sky_constants* sky, float out[10]);

/* ur_env_sky on the host, serial: the CPU fallback and the byte reference, over csrc/env_sky_rule.h, the very functions the kernel runs,
 * every texel's taps summed in the rule's 64-lane order. All pointers are host memory; no GPU is needed. The same refusals as ur_env_sky
 * but for the context. */
int ur_host_env_sky(const ur_sky_constants* sky, uint32_t base_size, uint32_t taps, void* dst_host, size_t dst_bytes);

/* The sample table of the BRDF LUT (include/ur_brdf_lut.h): for every row y of `height`, alpha = ((y + 0.5) / height)^2, the
 * GGX importance half vectors of the sample_count Hammersley points of ur_host_env_prefilter_table, (sin cos phi, sin sin phi, cos) with
 * cos^2 = (1 - xi2) / (1 + (alpha^2 - 1) xi2) and phi = 2 pi xi1, in double, each rounded to fp32: 16 bytes {hx, hy, hz, 0} a row and
 * sample, rows outer. The device reads these very bytes. Writes ur_brdf_lut_table_bytes(height, sample_count) bytes; UR_EINVAL for a
 * null out, numbers that function refuses or fewer out_bytes. */
int ur_host_brdf_lut_table(uint32_t height, uint32_t sample_count, void* out, size_t out_bytes);

/* ur_brdf_lut on the host, serial: the CPU fallback and the byte reference, over csrc/brdf_lut_rule.h, the very functions the kernel runs,
 * every texel's samples summed in the rule's 64-lane order. All pointers are host memory; no GPU is needed. The same refusals as
 * ur_brdf_lut but for the context. */
int ur_host_brdf_lut(uint32_t width, uint32_t height, uint32_t sample_count, const void* table_host, size_t table_bytes, void* dst_host, size_t dst_bytes);

/* A built-in debug-print font, so that ur_debug_print_draw / UR_FRAME_DEBUG_PRINT work with no asset (the reference bakes its atlas
 * from a font file with stb_truetype, DebugPrintFont.cpp; that stays the caller's). 5 x 7 dot-matrix glyphs of this repository's own
 * design for codes 32..95 in 8 x 8 cells of a 64 x 64 R8 atlas; glyph quad = the cell, Size (8, 8), Offset (0, -7), Advance 8
 * (kDebugPrintDefaultAdvance). info_out = {atlas_w, atlas_h, first_char, char_count} = {64, 64, 32, 64}; the glyph table is indexed by
 * code and has first_char + char_count = 96 entries (codes below 32 zero). atlas_out == glyphs_out == NULL: info_out only. UR_EINVAL
 * for a null info_out, one buffer without the other, atlas_capacity < atlas_w * atlas_h bytes or glyph_capacity < 96 entries. */
int ur_host_debug_font(uint8_t* atlas_out, uint32_t atlas_capacity, ur_debug_glyph* glyphs_out, uint32_t glyph_capacity, uint32_t info_out[4]);

/* Scene JSON conventions: BuildDirectionFromEulerDegrees (Scene/SceneJsonLoader.cpp:257-269); camera forward from
 * (pitch, yaw) degrees via RotationRollPitchYaw (Core/Application.cpp:896-902); and the light vector the renderer
 * ends up with after the app's asin/atan2 round trip (Core/Application.cpp:236-242,1225-1230), i.e. (d.x,-d.y,d.z). */
void ur_host_direction_from_euler_degrees(float pitch_deg, float yaw_deg, float out[3]);
void ur_host_camera_forward_from_euler_degrees(float pitch_deg, float yaw_deg, float out[3]);
void ur_host_light_direction_roundtrip(const float json_dir[3], float out[3]);

#ifdef __cplusplus
}
#endif
#endif /* UR_HOST_H */
