/*
 * ur_raster.h — C face of the raster passes: the ShadowMap pass (DeferredRenderer.cpp:551-633, Shaders/ShadowMap.hlsl), a depth-only
 * raster of indexed triangle lists under an orthographic light into an R32F map. The raster rule is DESIGN.md section 3.7; its numpy
 * restatement is tests/shadow_ref.py, and the two agree on every byte.
 * The DepthPrepass pass (DeferredRenderer.cpp:635-718, Shaders/DeferredBasePass.hlsl:58-70): the same raster under a perspective camera
 * with a near clip, reverse-Z, into the camera's depth buffer. Its rule is DESIGN.md section 3.8, restated in tests/depth_ref.py.
 */
#ifndef UR_RASTER_H
#define UR_RASTER_H

#include "ur_hotpath.h"

#ifdef __cplusplus
extern "C" {
#endif

#define UR_RASTER_MAX_TARGET 16384u  /* largest map width / height, and the guard band in pixels (D3D12_REQ_TEXTURE2D_U_OR_V_DIMENSION) */
#define UR_RASTER_INDEX_FORMAT_R32_UINT 42u /* DXGI_FORMAT_R32_UINT, the only index format drawn (RendererUtils.cpp:215) */

/* The draws of a raster pass: 64-byte FIndirectDrawCommand slots (RendererUtils.h:102-111) and which of them to draw.
 *   bytes  0-15  VertexBufferView  {u64 address, u32 size, u32 stride}; POSITION = three floats at byte 0 of a vertex
 *   bytes 16-31  IndexBufferView   {u64 address, u32 size, u32 format}
 *   bytes 32-39  ConstantBufferAddress: World = the first 64 bytes (row-vector convention, v' = v * World)
 *   bytes 40-59  IndexCountPerInstance, InstanceCount, StartIndexLocation, BaseVertexLocation (signed), StartInstanceLocation
 * On a HIP host the three addresses are device pointers. A selected slot is drawn when its InstanceCount (dword 11) is non-zero:
 * DrawIndexedInstanced(IndexCount, 1, StartIndex, BaseVertex, 0), triangle t = indices [Start + 3t, Start + 3t + 3); a trailing
 * one or two indices draw nothing. Selection, at most one of the two; neither = every slot of `commands`:
 *   visible_idx + visible_count: slots visible_idx[k] - index_base of `commands`, k < *visible_count (a camera's or a cull view's
 *       list); entries that fall outside [0, command_count) and k >= command_count are skipped;
 *   ranges: slots [offsets[r], offsets[r] + min(counts[r], offsets[r+1] - offsets[r])) of ranges->commands for every r (what a view's
 *       `draws` wrote); `commands` is then not read and may be NULL; slots >= command_count are skipped. */
typedef struct ur_raster_draws {
    const void* commands;          /* device, 16-byte aligned: command_count slots */
    uint32_t    command_count;     /* host: slots in `commands` (in ranges->commands with ranges) */
    const uint32_t* visible_idx;   /* device or NULL */
    const uint32_t* visible_count; /* device or NULL: both or neither */
    uint32_t    index_base;
    const ur_draw_ranges* ranges;  /* host struct of device pointers, or NULL */
} ur_raster_draws;

/* The ShadowMap pass: every texel of shadow_map (w x h floats, row-major, 4-byte aligned) is set to 1.0f, then the selected draws are
 * rasterised by the rule of DESIGN.md 3.7 (CULL_MODE_FRONT with FrontCounterClockwise, LESS_EQUAL, zero bias, depth clip): a texel
 * ends as the minimum depth of the fragments that cover its centre. The bytes do not depend on the order of anything.
 * light_view_projection: host, 16 floats, row-major, row-vector convention - scene->LightViewProjection as UpdateSceneConstants
 * writes it. Asynchronous on the context's stream; the host neither reads device memory nor synchronises; at most three launches
 * (clear, raster, and the large-triangle queue when ur_raster_reserve gave one).
 * stats4: device u32[4] or NULL, added to (the caller zeroes): [0] triangles rasterised (they passed every test below and face the
 * light's back: they may still cover no centre), [1] triangles skipped as unsupported - a vertex whose clip w is not exactly 1.0f,
 * a command whose index format is not R32_UINT, whose stride is below 12 or not a multiple of 4, whose addresses are null or not
 * 4-byte aligned, or an index / a vertex that lies outside its buffer view -, [2] triangles dropped for a non-finite coordinate or a
 * vertex outside the guard band (|X| or |Y| > 16384 px), [3] large triangles that did not fit the reserved queue and were rasterised
 * by the wave that found them (slow, never wrong).
 * UR_EUNSUPPORTED, nothing launched: the matrix's fourth column is not exactly (0, 0, 0, 1) (a perspective light).
 * UR_EINVAL, nothing launched: a null context, matrix, draws or map; commands null with command_count != 0 and no ranges; a buffer
 * that is not aligned (commands 16, the rest 4 bytes); w or h 0 or above 16384; both selections; a list without its count or a count
 * without its list; a null member of ranges or range_count == 0. */
int ur_shadow_map(ur_ctx* ctx, const float light_view_projection[16], const ur_raster_draws* draws,
                  float* shadow_map, uint32_t w, uint32_t h, uint32_t* stats4);

/* Room for max_large_work_items (triangle, 64 x 64 tile) entries of the large-triangle queue of this context: a triangle whose
 * bounding box covers more than 64 8 x 8 stamps is split over the tiles it touches and rasterised by a second launch. 0 frees the
 * queue. Optional for correctness: without room every large triangle is rasterised where it is found and counted in stats4[3].
 * Synchronises the context's stream when it has to replace a queue (call it at set-up). UR_ENOMEM when the allocation fails. */
int ur_raster_reserve(ur_ctx* ctx, uint32_t max_large_work_items);

#define UR_DEPTH_QUANTIZE_D24 0x1u /* every fragment stores (float)(rint((double)z * 16777215.0) / 16777215.0): a D24_UNORM target read through its R24 view */
#define UR_DEPTH_GUARD_BAND 2097152u /* the DepthPrepass guard band in pixels (2^21): snapped coordinates stay below 2^29 */

/* The DepthPrepass pass: every texel of depth (w x h floats, row-major, 4-byte aligned) is set to 0.0f, then the selected draws are
 * rasterised by the rule of DESIGN.md 3.8 (position * World * View * Projection, the near clip z <= w, CULL_MODE_BACK with
 * FrontCounterClockwise, GREATER_EQUAL on a reverse-Z target): a texel ends as the maximum depth, clamped to 1.0f, of the fragments that
 * cover its centre. The bytes do not depend on the order of anything.
 * view, projection: host, 16 floats each, row-major, row-vector convention - scene->View and scene->Projection; they are multiplied
 * per vertex in that order, never with each other. Asynchronous on the context's stream; the host neither reads device memory nor
 * synchronises; at most three launches (clear, raster, and the large-triangle queue when ur_raster_reserve gave one).
 * Read: the selected command slots; of each drawn slot its index range, the 12 POSITION bytes of the vertices that range names and
 * the first 64 bytes behind ConstantBufferAddress; visible_count[0] and the list entries in front of it, or the ranges' offsets and
 * counts. Nothing else of these buffers is read, and none of them is written.
 * Written: all w * h floats of depth, and nothing around them. stats6 is added to. The large-triangle queue is the context's own.
 * flags: UR_DEPTH_QUANTIZE_D24 or 0.
 * stats6: device u32[6] or NULL, added to (the caller zeroes): [0] emitted triangles rasterised (they passed every test below and
 * face the camera: they may still cover no centre), [1] triangles skipped as unsupported - a vertex with a non-finite clip coordinate
 * or clip z <= 0 (a projection that is not reverse-Z with an infinite far plane), and the command, index and vertex cases of
 * ur_shadow_map -, [2] emitted triangles dropped for a non-finite target coordinate or a vertex outside the guard band (|X| or |Y| >
 * 2^21 px: side planes are not clipped, the caller splits such triangles), [3] large triangles that did not fit the reserved queue
 * and were rasterised by the wave that found them, [4] triangles cut by the near plane (one or two vertices behind it; one behind
 * emits two triangles), [5] triangles wholly behind the near plane.
 * UR_EINVAL, nothing launched: ur_shadow_map's cases (with view, projection and depth for the matrix and the map), and flag bits
 * other than UR_DEPTH_QUANTIZE_D24. */
int ur_depth_prepass(ur_ctx* ctx, const float view[16], const float projection[16], const ur_raster_draws* draws,
                     float* depth, uint32_t w, uint32_t h, uint32_t flags, uint32_t* stats6);

#ifdef __cplusplus
}
#endif
#endif /* UR_RASTER_H */
