/*
 * ur_raster.h — C face of the raster passes: the ShadowMap pass (DeferredRenderer.cpp:551-633, Shaders/ShadowMap.hlsl), a depth-only
 * raster of indexed triangle lists under an orthographic light into an R32F map. The raster rule is DESIGN.md section 3.7; its numpy
 * restatement is tests/shadow_ref.py, and the two agree on every byte.
 * The DepthPrepass pass (DeferredRenderer.cpp:635-718, Shaders/DeferredBasePass.hlsl:58-70): the same raster under a perspective camera
 * with a near clip, reverse-Z, into the camera's depth buffer. Its rule is DESIGN.md section 3.8, restated in tests/depth_ref.py.
 * The GBuffer pass (DeferredRenderer.cpp:720-865, Shaders/DeferredBasePass.hlsl, pipeline key 0: no texture maps, no alpha mask) and the
 * ObjectId pass (:867-980, Shaders/ObjectId.hlsl): DepthPrepass' raster writing a visibility key per texel, and a per-texel resolve of
 * the winning key into the render targets. Its rule is DESIGN.md section 3.9, restated in tests/gbuffer_ref.py. Texture maps (pipeline
 * keys 0-15) are section 3.10 and tests/gbuffer_tex_ref.py, the alpha-masked permutations (keys 16-31) section 3.11 and
 * tests/gbuffer_mask_ref.py.
 * The Forward pass (ForwardRenderer.cpp "Forward", Shaders/ForwardVS.hlsl, Shaders/ForwardPS.hlsl): the same visibility keys resolved
 * straight to the HDR colour. Its rule is DESIGN.md section 3.12, restated in tests/forward_ref.py.
 * The ObjectId pass of both renderers as a call of its own over any draws and any depth, and the pick of up to 64 texels without an
 * image: DESIGN.md section 3.16, restated in tests/object_id_ref.py.
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
 * Synchronises the context's stream when it has to replace a queue (call it at set-up). UR_ENOMEM when the allocation fails.
 * The allocation is 64 bytes per entry + 64: the 48 bytes a depth pass writes per entry, and 16 more that only ur_gbuffer_pass uses (the
 * triangle's key), since one queue serves all three passes. Before ur_gbuffer_pass existed an entry cost 48 bytes: a caller of
 * ur_shadow_map and ur_depth_prepass alone now pays a third more device memory for the same count (32 MiB instead of 24 at 2^19). */
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

/* The targets of the GBuffer pass: the rows [row0, row0 + rows) of the frame, w texels wide, row-major (a band's own images). */
typedef struct ur_gbuffer_targets {
    ur_half4* gbuf_a; ur_half4* gbuf_b; uint32_t* gbuf_c; ur_half4* hdr;   /* rows [row0,row0+rows), w wide */
    uint32_t* object_id;   /* nullable */
    uint32_t* keys;        /* rows x w scratch owned by the caller; holds the winning keys afterwards */
} ur_gbuffer_targets;

/* The GBuffer pass (and, with targets->object_id, the ObjectId pass) over the rows [row0, row0 + rows) of a w x h frame, by the rule
 * of DESIGN.md 3.9. The selected draws are rasterised exactly as ur_depth_prepass rasterises them (vertex, near clip, viewport, facing,
 * coverage, depth plane, UR_DEPTH_QUANTIZE_D24); a fragment passes iff its value is >= depth[texel] (GREATER_EQUAL, depth is never
 * written), and a texel of `keys` ends as the maximum key over its passing fragments: triangle t of the draw of ordinal o has the key
 * ((o + 1) << T) | t, 0 = nothing; o is the slot index (every slot, ranges) or the position in the visible list, so among equal depths
 * the draw and triangle that D3D draws last wins. T = key_triangle_bits, or 32 - bit_length(command_count) when that is 0. A resolve
 * launch then writes EVERY texel of the band's targets: key 0 gives the clear values - gbuf_a = gbuf_b = hdr = fp16 (0, 0, 0, 1),
 * gbuf_c = 0xFF000000, object_id = 0 -, any other key the base pass' pixel shader on perspective-correct attributes of that triangle:
 * gbuf_a = fp16 (view normal, view depth), gbuf_b = fp16 (0.04, MetallicFactor, RoughnessFactor, 1), gbuf_c = sRGB8 of BaseColor *
 * COLOR.rgb (R in the low byte, alpha byte 255; ur_host_srgb_encode_table), hdr = fp16 (EmissiveFactor, 1), object_id = ObjectId.
 * With `depth` the result of ur_depth_prepass over the same draws, matrices and flags this is the reference's G-buffer. With any other
 * depth it is still defined by the rule, but it is not that picture: a texel whose depth is above every fragment stays clear, one
 * whose depth is below several fragments takes the last drawn of them, not the nearest.
 * A vertex is 64 bytes: POSITION at byte 0, NORMAL at 12, TEXCOORD at 24, TANGENT at 32, COLOR at 48 (DeferredRenderer.cpp:1812-1816).
 * ConstantBufferAddress points at a whole ur_scene_constants: World, BaseColor, EmissiveFactor, MetallicFactor, RoughnessFactor and
 * ObjectId are read from it; view and projection come from the host as for ur_depth_prepass.
 * Asynchronous on the context's stream; the host neither reads device memory nor synchronises; at most four launches (clear of the
 * keys, raster, the large-triangle queue when ur_raster_reserve gave one, resolve).
 * Read: what ur_depth_prepass reads, with all 64 bytes of a named vertex and the 608 bytes behind ConstantBufferAddress; the w * h floats
 * of depth (only rows [row0, row0 + rows) of them). None of these is written.
 * Written: rows * w elements of gbuf_a, gbuf_b, gbuf_c, hdr, keys and (when given) object_id, every one of them, and nothing around
 * them. stats6 is added to.
 * stats6: ur_depth_prepass' meanings; [1] also counts every triangle of a command whose stride is below 64 or that has more than 2^T
 * triangles (neither is drawn), and a triangle with a vertex whose 64 bytes do not lie inside its buffer view. Triangles are counted
 * whether or not they touch the band.
 * UR_EINVAL, nothing launched: ur_depth_prepass' cases; null targets or a null target other than object_id; a misaligned target
 * (gbuf_a, gbuf_b, hdr 8 bytes, the others 4); rows == 0 or row0 + rows > h; key_triangle_bits > 31; command_count >= 2^(32 - T).
 * UR_EUNSUPPORTED, nothing launched: key_triangle_bits == 0 with command_count >= 2^24. */
int ur_gbuffer_pass(ur_ctx* ctx, const float view[16], const float projection[16], const ur_raster_draws* draws,
                    const float* depth, const ur_gbuffer_targets* targets, uint32_t w, uint32_t h, uint32_t row0, uint32_t rows,
                    uint32_t flags, uint32_t key_triangle_bits, uint32_t* stats6);

#define UR_GBUFFER_PART_RASTER 0x1u  /* the clear of the keys, the raster and the large-triangle queue */
#define UR_GBUFFER_PART_RESOLVE 0x2u /* the resolve */

/* ur_gbuffer_pass in parts, for tools that time its two halves apart (tools/bench_shadow.py --pass gbuffer); ur_gbuffer_pass is this
 * call with both parts. UR_GBUFFER_PART_RASTER alone launches the clear, the raster and the queue: it reads what ur_gbuffer_pass reads
 * except the NORMAL..COLOR bytes of a vertex and the constants behind World, writes the rows * w keys and adds to stats6; the other
 * targets are not touched. UR_GBUFFER_PART_RESOLVE alone launches the resolve over the keys as they are: they must be what the raster
 * part left under the same draws, matrices, band, flags and key_triangle_bits (a key that names no triangle of these draws reads
 * outside the caller's buffers); it reads the keys, the draws' buffers and the list, not depth, and writes the other targets; stats6 is
 * not touched. Arguments, checks and return values are ur_gbuffer_pass', all of them in either part; parts == 0 or an unknown bit is
 * UR_EINVAL. */
int ur_gbuffer_pass_parts(ur_ctx* ctx, const float view[16], const float projection[16], const ur_raster_draws* draws,
                          const float* depth, const ur_gbuffer_targets* targets, uint32_t w, uint32_t h, uint32_t row0, uint32_t rows,
                          uint32_t flags, uint32_t key_triangle_bits, uint32_t* stats6, uint32_t parts);

#define UR_TEXTURE_R8G8B8A8_UNORM 28u      /* DXGI_FORMAT_R8G8B8A8_UNORM */
#define UR_TEXTURE_R8G8B8A8_UNORM_SRGB 29u /* DXGI_FORMAT_R8G8B8A8_UNORM_SRGB: R, G and B decode through ur_host_srgb_decode_table, alpha never */

/* The block-compressed formats: a texel is the RGBA8 code word that the integer rule of 3.13 decodes from its 4 x 4
 * block, and everything behind the code word is the RGBA8 formats'. BC2, BC4, BC6H, BC7 and the SNORM forms are not sampled. (The values
 * stand in parentheses as UR_MATERIAL_ALPHA_MASK's does: tests/test_gbuffer_tex_abi.py pins the list of bare ones.) */
#define UR_TEXTURE_BC1_UNORM (71u)    /* DXGI_FORMAT_BC1_UNORM: 8-byte blocks; index 3 of a block with c0 <= c1 is (0, 0, 0, 0) */
#define UR_TEXTURE_BC1_UNORM_SRGB (72u) /* DXGI_FORMAT_BC1_UNORM_SRGB */
#define UR_TEXTURE_BC3_UNORM (77u)    /* DXGI_FORMAT_BC3_UNORM: 16-byte blocks, an alpha block in front of a four-colour block */
#define UR_TEXTURE_BC3_UNORM_SRGB (78u) /* DXGI_FORMAT_BC3_UNORM_SRGB */
#define UR_TEXTURE_BC5_UNORM (83u)    /* DXGI_FORMAT_BC5_UNORM: 16-byte blocks, R and G; B = 0, A = 255 */

/* A texture of the textured GBuffer resolve: `mips` levels packed tightly one behind the other from `texels` (device, 4-byte aligned),
 * level k = max(1, width >> k) x max(1, height >> k) texels of 4 bytes, row-major, R in the low byte. Any size 1..65535, powers of two
 * or not. `mips` may be anything 1..255: levels past the end of the chain (every level from 16 on) are 1 x 1 texels packed one behind
 * the other like any level.
 * A BC format: level k has the same wk = max(1, width >> min(k, 16)) by hk = max(1, height >> min(k, 16)) texels, stored as
 * ((wk + 3) >> 2) x ((hk + 3) >> 2) blocks, row-major, 8 bytes a block for BC1 and 16 for BC3 and BC5; the levels follow each other with
 * no padding - the order and pitch of a DDS file's mip chain, so a file's payload is the device buffer - and every level from 16 on is
 * one block. Texel (x, y) lies in block (x >> 2, y >> 2) at index 4 * (y & 3) + (x & 3). Wrap addressing stays in texels over wk, hk: the
 * padding texels of an edge block are never selected. `texels` is then aligned to the block size, 8 or 16 bytes
 * (ur_host_bc_chain_bytes gives the chain's size). */
typedef struct ur_texture2d {
    uint64_t texels;
    uint16_t width, height;
    uint8_t  mips, format;
    uint16_t reserved;
} ur_texture2d; /* 16 bytes */

/* Transcode at load time: a chain of block-compressed levels becomes the RGBA8 chain the sampler is fastest on, on the
 * device. The sources are the five BC codes above and the five below - ten in all. The five below are transcode sources only, never
 * ur_texture2d.format values: a descriptor that carries one is invalid as before. (Values in parentheses, as above.) */
#define UR_TEXTURE_SOURCE_BC2_UNORM (74u)      /* DXGI_FORMAT_BC2_UNORM: 16 four-bit alphas (A = a * 17) in front of a four-colour block */
#define UR_TEXTURE_SOURCE_BC2_UNORM_SRGB (75u) /* DXGI_FORMAT_BC2_UNORM_SRGB */
#define UR_TEXTURE_SOURCE_BC4_UNORM (80u)      /* DXGI_FORMAT_BC4_UNORM: 8-byte blocks, R; G = B = 0, A = 255 */
#define UR_TEXTURE_SOURCE_BC7_UNORM (98u)      /* DXGI_FORMAT_BC7_UNORM: 16-byte blocks, the BPTC rule; the reserved mode is (0, 0, 0, 0) */
#define UR_TEXTURE_SOURCE_BC7_UNORM_SRGB (99u) /* DXGI_FORMAT_BC7_UNORM_SRGB */

/* Bytes of the RGBA8 chain of a width x height texture with `mips` levels: 4 bytes a texel, level k = max(1, width >> min(k, 16)) by
 * max(1, height >> min(k, 16)), tightly packed. Host only. 0 for a zero dimension, a dimension above 65535, or mips outside 1..255. */
uint64_t ur_texture_transcode_bytes(uint32_t width, uint32_t height, uint32_t mips);
/* Decode the chain at `blocks` (device; the BC layout above, 8 bytes a block for BC1 and BC4 and 16 for the rest;
 * ur_host_texture_chain_bytes gives its size) into the RGBA8 chain at `rgba8` (device, ur_texture_transcode_bytes bytes): every texel
 * becomes its RGBA8 code word, R in the low byte, the _SRGB forms giving their UNORM twins' code words. One launch on the context's
 * stream, asynchronous: the host neither reads device memory nor synchronises. Reads exactly the source chain's bytes and writes
 * exactly the destination chain's; the padding texels of edge blocks are never written.
 * out_descriptor (host, nullable) is filled with {rgba8, width, height, mips, UR_TEXTURE_R8G8B8A8_UNORM_SRGB for the sources 72, 75,
 * 78 and 99, else UR_TEXTURE_R8G8B8A8_UNORM}: what ur_material takes.
 * UR_EINVAL, nothing launched: a null context, blocks or rgba8; a source_format outside the ten; blocks not aligned to the block size
 * (8 or 16 bytes); rgba8 not 4-byte aligned; a zero dimension, a dimension above 65535, mips outside 1..255; source and destination
 * sharing a byte. */
int ur_texture_transcode(ur_ctx* ctx, uint32_t source_format, const void* blocks, uint32_t width, uint32_t height, uint32_t mips, void* rgba8,
                         ur_texture2d* out_descriptor);

#define UR_MATERIAL_NORMAL_MAP 0x1u             /* BuildPipelineKey (DeferredRenderer.cpp:28-36): USE_NORMAL_MAP, texture t2 */
#define UR_MATERIAL_METALLIC_ROUGHNESS_MAP 0x2u /* USE_METALLIC_ROUGHNESS_MAP, t1 */
#define UR_MATERIAL_BASE_COLOR_MAP 0x4u         /* USE_BASE_COLOR_MAP, t0 */
#define UR_MATERIAL_EMISSIVE_MAP 0x8u           /* USE_EMISSIVE_MAP, t3 */

#define UR_MATERIAL_ALPHA_MASK (0x10u)          /* USE_ALPHA_MASK: looked at by ur_gbuffer_pass_masked only, for the draws of its mask */

/* What the reference binds per draw range (DeferredRenderer.cpp:800): the descriptor table t0-t3 and the pipeline key. One record per
 * command slot. Key bits 4 and above are ignored in ur_gbuffer_pass, _parts, _materials and _materials_parts (USE_ALPHA_MASK is not drawn
 * by them: the caller's ranges keep such models out, or go to ur_gbuffer_pass_masked); bits 5 and above are ignored everywhere. A set bit is
 * treated as clear when its texture has a null address, an address that is not aligned to 4 bytes (RGBA8), 8 (BC1) or 16 (BC3, BC5), a zero
 * dimension, zero mips or a format other than the seven above. */
typedef struct ur_material {
    ur_texture2d base_color, metallic_roughness, normal, emissive; /* t0, t1, t2, t3 */
    uint32_t pipeline_key;
    uint32_t reserved[3];
} ur_material; /* 80 bytes, 16-byte aligned */

/* ur_gbuffer_pass with texture maps: pipeline keys 0-15 of DeferredBasePass.hlsl by the rule of DESIGN.md 3.10, restated in
 * tests/gbuffer_tex_ref.py. The raster is ur_gbuffer_pass'; the resolve of a texel whose winning key names command slot s evaluates the
 * pixel shader under materials[s].pipeline_key: each map is sampled at its own ApplyTextureTransform of the interpolated TEXCOORD with
 * the base pass' static sampler (anisotropic, MaxAnisotropy 4, wrap, every mip, no LOD bias) as 3.10 defines it - derivatives from the
 * texel's 2 x 2 quad partners on its own triangle, up to four trilinear probes along the major axis. gbuf_a's normal goes through
 * ComputeViewNormal with the interpolated TANGENT, gbuf_c's albedo is multiplied by the base-colour sample's rgb, gbuf_b's metallic and
 * roughness by the metallic-roughness sample's b and g, hdr's emissive by the emissive sample's rgb. Key 0 gives ur_gbuffer_pass' bytes.
 * materials: device, 16-byte aligned, material_count records; NULL is ur_gbuffer_pass (material_count is then not looked at). A slot
 * >= material_count resolves as key 0.
 * Read: what ur_gbuffer_pass reads; materials[s] (80 bytes) for every slot s < material_count that a winning key names; of a texture
 * whose bit is set and whose descriptor is valid, 4-byte texels - of a BC format whole 8- or 16-byte blocks - inside the bytes of its
 * `mips` levels (width, height, mips and format as the record gives them) and nothing around them. None of these is written.
 * Written, launches, stats6: ur_gbuffer_pass'.
 * UR_EINVAL, nothing launched: ur_gbuffer_pass' cases; materials not 16-byte aligned. */
int ur_gbuffer_pass_materials(ur_ctx* ctx, const float view[16], const float projection[16], const ur_raster_draws* draws,
                              const float* depth, const ur_gbuffer_targets* targets, uint32_t w, uint32_t h, uint32_t row0, uint32_t rows,
                              uint32_t flags, uint32_t key_triangle_bits, uint32_t* stats6, const ur_material* materials, uint32_t material_count);

/* ur_gbuffer_pass_materials in parts, as ur_gbuffer_pass_parts: the raster part reads no material, the resolve part reads them. */
int ur_gbuffer_pass_materials_parts(ur_ctx* ctx, const float view[16], const float projection[16], const ur_raster_draws* draws,
                                    const float* depth, const ur_gbuffer_targets* targets, uint32_t w, uint32_t h, uint32_t row0, uint32_t rows,
                                    uint32_t flags, uint32_t key_triangle_bits, uint32_t* stats6, uint32_t parts,
                                    const ur_material* materials, uint32_t material_count);

/* The alpha-masked draws of ur_gbuffer_pass_masked. */
typedef struct ur_gbuffer_mask {
    const ur_raster_draws* draws; /* the alpha-masked selection; same commands / command_count as the opaque one */
    uint64_t* keys64;             /* rows x w scratch, 8-byte aligned, owned by the caller */
    uint32_t* stats6;             /* nullable, added to: ur_depth_prepass' meanings for the masked draws */
    uint32_t* won;                /* nullable, added to: texels whose final key is a masked fragment's */
} ur_gbuffer_mask;

/* ur_gbuffer_pass_materials with the alpha-masked permutations, pipeline keys 16-31 of DeferredBasePass.hlsl ("GBuffer" under
 * BasePassPipelines[16..31], depth write on: DeferredRenderer.cpp:1862-1864), by the rule of DESIGN.md 3.11, restated in
 * tests/gbuffer_mask_ref.py. `draws` are the opaque models, drawn exactly as ur_gbuffer_pass_materials draws them, against `depth` (the
 * prepass of the opaque models only, as in the reference) into targets->keys. mask->draws are the masked models, a second selection over
 * the same commands and command_count, so that the keys of both share one space. A masked fragment is rasterised like any other and
 * passes iff its depth is >= depth[texel] as the call found it; when bit 4 (UR_MATERIAL_ALPHA_MASK) of its slot's pipeline_key is set it
 * is discarded iff alpha < AlphaCutoff, alpha = BaseColorAlpha * interpolated COLOR.a (vertex byte 60), times channel A of the base-colour
 * map (code / 255, never decoded; the resolve's sampler at the resolve's coordinates and derivatives) when bit 2 is set and the
 * descriptor is valid. AlphaMode in the constants is not consulted; a slot >= material_count, or materials == NULL, has key 0: nothing of
 * it is discarded. Per texel the surviving masked fragment of the greatest depth wins, the greatest key among equal depths; it replaces
 * the opaque key iff its depth is above depth[texel], or its key above the opaque key (it passed, so its depth is not below). Where it
 * does, depth[texel] is raised to its depth - the depth buffer the reference's "GBuffer" pass leaves for "Build HZB" - and
 * mask->keys64[texel] keeps (depth bits << 32) | key; everywhere else in the band keys64 ends as 0. The resolve then runs over the final
 * keys; the pixel shader behind the alpha test is that of the key without bit 4.
 * With visible lists the ordinal of a key is the position in its own selection's list: a tie between the two selections at exactly equal
 * depth is decided by the key's value, which is D3D's draw order only for the slot-indexed selections (every slot, ranges). The resolve
 * then tells the selections apart by keys64.
 * mask == NULL is ur_gbuffer_pass_materials: depth is then not written. Either selection may select nothing, and command_count may be 0.
 * Asynchronous on the context's stream; the host neither reads device memory nor synchronises; at most eight launches (clear, raster and
 * large-triangle queue of the opaque draws, the same three of the masked draws - the queue is reused in stream order -, merge, resolve).
 * Read: what ur_gbuffer_pass_materials reads, for both selections; materials[s] for every slot s < material_count of a masked fragment
 * that passes the depth test; of a masked draw's textures the raster reads the base-colour chain only (4-byte texels, or whole BC blocks,
 * inside the bytes of its `mips` levels; nothing of a BC5 chain), the resolve what ur_gbuffer_pass_materials' reads; TEXCOORD and COLOR.a (bytes 24-31 and 60-63) of such a fragment's vertices and
 * the constants behind ConstantBufferAddress.
 * Written: ur_gbuffer_pass_materials' targets; all rows * w words of keys64; of depth only rows [row0, row0 + rows), and of those only
 * the texels that `won` counts. stats6 counts the opaque draws, mask->stats6 the masked ones, mask->won is added to.
 * UR_EINVAL, nothing launched: ur_gbuffer_pass_materials' cases for both selections; a null mask->draws; a null keys64 or one that is not
 * 8-byte aligned; a misaligned mask->stats6 or won; mask->draws over other commands or another command_count than draws; keys64
 * overlapping a target or depth.
 * UR_EUNSUPPORTED, nothing launched: targets->object_id together with a mask (the reference's ObjectId pass ignores the alpha test and
 * tests against the depth this pass writes: it needs a raster of its own - ur_object_id_pass below, over the depth this call leaves). */
int ur_gbuffer_pass_masked(ur_ctx* ctx, const float view[16], const float projection[16], const ur_raster_draws* draws,
                           float* depth, const ur_gbuffer_targets* targets, uint32_t w, uint32_t h, uint32_t row0, uint32_t rows,
                           uint32_t flags, uint32_t key_triangle_bits, uint32_t* stats6, const ur_material* materials, uint32_t material_count,
                           const ur_gbuffer_mask* mask);

/* ur_gbuffer_pass_masked in parts, as ur_gbuffer_pass_parts: UR_GBUFFER_PART_RASTER is the six raster launches and the merge (it writes
 * keys, keys64 and depth), UR_GBUFFER_PART_RESOLVE the resolve over keys and keys64 as that part left them. */
int ur_gbuffer_pass_masked_parts(ur_ctx* ctx, const float view[16], const float projection[16], const ur_raster_draws* draws,
                                 float* depth, const ur_gbuffer_targets* targets, uint32_t w, uint32_t h, uint32_t row0, uint32_t rows,
                                 uint32_t flags, uint32_t key_triangle_bits, uint32_t* stats6, uint32_t parts,
                                 const ur_material* materials, uint32_t material_count, const ur_gbuffer_mask* mask);

/* The targets of the Forward pass: the rows [row0, row0 + rows) of the frame, w texels wide, row-major (a band's own images). */
typedef struct ur_forward_targets {
    ur_half4* hdr;   /* the HDR band: written where a key won, left as it is elsewhere */
    uint32_t* keys;  /* rows x w scratch owned by the caller; holds the winning keys afterwards */
} ur_forward_targets;

/* The Forward pass (ForwardRenderer.cpp "Forward", Shaders/ForwardVS.hlsl and ForwardPS.hlsl, all 32 pipeline permutations) over the rows
 * [row0, row0 + rows) of a w x h frame, by the rule of DESIGN.md 3.12, restated in tests/forward_ref.py. The raster is
 * ur_gbuffer_pass_masked's, unchanged: keys, keys64, depth, won and both stats6 end exactly as that call leaves them. A second resolve over
 * the final keys then evaluates material and lighting in one go, from fp32 values: where the key is not 0, hdr = fp16 (color.rgb, 1.0) of
 * ForwardPS.hlsl:73-143 on the perspective-correct attributes of the key's triangle; every other texel of hdr is left untouched (the
 * reference draws "Sky" first and "Forward" over it: call ur_sky_atmosphere on the band first). The maps are sampled with 3.10's sampler,
 * the metallic-roughness map at the base-colour map's transform (ForwardPS.hlsl:103); the shadow map, the staged cube and the BRDF LUT are
 * filtered as ur_deferred_lighting's definitions say (3.12 lists them).
 * Constants. Per draw, from the 608 bytes behind each command's ConstantBufferAddress: World, BaseColor, EmissiveFactor, MetallicFactor,
 * RoughnessFactor, BaseColorAlpha, AlphaCutoff and the BaseColor, Normal and Emissive texture transforms. Per frame, from frame_constants on
 * the host: LightDirection, LightColor, LightIntensity, CameraPosition, LightViewProjection, ShadowStrength, ShadowBias, ShadowMapSize and
 * EnvMapMipCount; its other fields are not read, and a command's copies of these nine are not read either. view and projection come from
 * the host as for ur_depth_prepass.
 * mask == NULL: the opaque raster alone (ur_gbuffer_pass_materials' keys), and depth is not written. materials == NULL: pipeline key 0 for
 * every slot.
 * Asynchronous on the context's stream; the host neither reads device memory nor synchronises; at most eight launches (ur_gbuffer_pass_masked's
 * seven raster and merge launches, and the forward resolve).
 * Read: what ur_gbuffer_pass_masked reads (the resolve reads the keys, keys64 under visible lists, the named vertices' 64 bytes, the constants
 * and the valid maps of the winning slots: 4-byte texels, or whole BC blocks, inside the bytes of their chains); of tables->shadow_map, when ShadowStrength > 0, floats inside its ShadowMapSize.x * ShadowMapSize.y;
 * of tables->env_cube the bordered faces (the first section of what ur_stage_env_cube wrote); of tables->brdf_lut_rg16 its lut_width *
 * lut_height texels. None of these is written.
 * Written: all rows * w keys; of hdr only the texels whose final key is not 0; with a mask, keys64 and depth as ur_gbuffer_pass_masked writes
 * them. stats6, mask->stats6 and mask->won are added to.
 * UR_EINVAL, nothing launched: ur_gbuffer_pass_masked's cases (with hdr and keys for the targets: null targets, a null or misaligned hdr
 * (8 bytes) or keys (4)); null tables or frame_constants; ShadowStrength > 0 with a null shadow_map or a ShadowMapSize outside 1..16384; a
 * null or misaligned env_cube or brdf_lut_rg16; env_base_size, env_mip_count, lut_width or lut_height 0, or more than 16 mips; an
 * env_cube_texels that is not ur_env_cube_texels(env_base_size, env_mip_count); hdr or keys overlapping each other, depth, the commands, the
 * material table, the shadow map, the staged cube, the LUT or keys64.
 * UR_EUNSUPPORTED, nothing launched: key_triangle_bits == 0 with command_count >= 2^24. */
int ur_forward_pass(ur_ctx* ctx, const float view[16], const float projection[16], const ur_raster_draws* draws,
                    float* depth, const ur_forward_targets* targets, uint32_t w, uint32_t h, uint32_t row0, uint32_t rows,
                    uint32_t flags, uint32_t key_triangle_bits, uint32_t* stats6, const ur_material* materials, uint32_t material_count,
                    const ur_gbuffer_mask* mask, const ur_scene_constants* frame_constants, const ur_lighting_tables* tables);

/* ur_forward_pass in parts, as ur_gbuffer_pass_masked_parts: UR_GBUFFER_PART_RASTER is the raster launches and the merge (hdr is not
 * touched), UR_GBUFFER_PART_RESOLVE the forward resolve over keys and keys64 as that part left them (tools/bench_shadow.py --pass forward).
 * Arguments, checks and return values are ur_forward_pass', all of them in either part; parts == 0 or an unknown bit is UR_EINVAL. */
int ur_forward_pass_parts(ur_ctx* ctx, const float view[16], const float projection[16], const ur_raster_draws* draws,
                          float* depth, const ur_forward_targets* targets, uint32_t w, uint32_t h, uint32_t row0, uint32_t rows,
                          uint32_t flags, uint32_t key_triangle_bits, uint32_t* stats6, uint32_t parts,
                          const ur_material* materials, uint32_t material_count, const ur_gbuffer_mask* mask,
                          const ur_scene_constants* frame_constants, const ur_lighting_tables* tables);

/* The ObjectId pass of either renderer (DeferredRenderer.cpp:867-980, ForwardRenderer.cpp:782-890, Shaders/ObjectId.hlsl, pipeline at
 * RendererUtils.cpp:692-760) as a call of its own, over any draws and any depth: DESIGN.md 3.16, restated in tests/object_id_ref.py. The
 * rule is ur_gbuffer_pass' (3.9) and nothing in it is new: every selected draw - opaque and alpha-masked models in ONE selection, as the
 * reference loops over all its models - is rasterised exactly as ur_depth_prepass rasterises it; there is no alpha test; a fragment passes
 * iff its value is >= depth[texel] (GREATER_EQUAL, depth is never written); a texel of `keys` ends as the maximum key over its passing
 * fragments, 0 = nothing - under the slot-indexed selections (every slot, ranges) the draw D3D draws last -; object_id[texel] is ObjectId
 * (dword 148) of the winning command's constants, 0 for key 0.
 * With the depth ur_gbuffer_pass_masked or ur_forward_pass left behind (or ur_depth_prepass' for opaque models) this is the reference's
 * ObjectId picture, its quirk included: a masked fragment that the base pass discarded in front of the visible surface still passes
 * GREATER_EQUAL here, so a pick through a hole of a masked model that is drawn later than the surface seen through it returns the masked
 * model, not that surface.
 * Asynchronous on the context's stream; the host neither reads device memory nor synchronises; at most four launches (clear of the keys,
 * raster, the large-triangle queue when ur_raster_reserve gave one, resolve).
 * Read: what ur_depth_prepass reads, with all 64 bytes of a named vertex's stride checked as ur_gbuffer_pass checks them and dword 148
 * behind the ConstantBufferAddress of a winning command; rows [row0, row0 + rows) of depth. None of these is written.
 * Written: all rows * w words of keys and of object_id, every one of them, and nothing around them; keys ends as ur_gbuffer_pass leaves it.
 * stats6 is added to, with ur_gbuffer_pass' meanings.
 * UR_EINVAL, nothing launched: ur_gbuffer_pass' cases (the targets being object_id and keys: either null or not 4-byte aligned);
 * object_id or keys overlapping depth, the commands or each other.
 * UR_EUNSUPPORTED, nothing launched: key_triangle_bits == 0 with command_count >= 2^24. */
int ur_object_id_pass(ur_ctx* ctx, const float view[16], const float projection[16], const ur_raster_draws* draws,
                      const float* depth, uint32_t* object_id, uint32_t* keys,
                      uint32_t w, uint32_t h, uint32_t row0, uint32_t rows,
                      uint32_t flags, uint32_t key_triangle_bits, uint32_t* stats6);

#define UR_PICK_MAX_POINTS 64u /* the most points of one ur_object_id_pick */

/* What ur_object_id_pick answers for one point. */
typedef struct ur_pick_result {
    uint32_t object_id;  /* ur_object_id_pass' object_id at the texel */
    uint32_t key;        /* ... and its key; 0 = nothing */
    uint32_t slot;       /* the command slot the key names; 0xFFFFFFFF for key 0 */
    uint32_t depth_bits; /* the bits of the winning fragment's depth (the value the depth test compared, after D24); 0 for key 0 */
} ur_pick_result; /* 16 bytes */

/* The pick: ur_object_id_pass' answer at up to UR_PICK_MAX_POINTS texels of the whole w x h frame, from the triangles alone - no key
 * image, no clear of one and no fragments other than the points' (DESIGN.md 3.16). Point i is (min(x, w - 1), min(y, h - 1)) of
 * points_xy[2 i], points_xy[2 i + 1] (the reference's clamp, DeferredRenderer.cpp:945-946); results[i] is exactly what ur_object_id_pass
 * over the same draws, matrices, depth, flags and key_triangle_bits gives at that texel, with the slot and the depth of the fragment that
 * won (the greatest among the winning key's fragments there). Equal points get equal records.
 * points_xy: host, read before the call returns. results: device, 16-byte aligned, point_count records.
 * Asynchronous on the context's stream; the host neither reads device memory nor synchronises; three stream operations (a clear of the
 * records, the pick, a one-wave finish), none when point_count == 0 (UR_OK; points_xy and results may then be NULL). The cost does not
 * depend on w * h.
 * Read: what ur_object_id_pass reads of the draws; of depth the floats at the clamped points only. Written: the point_count records,
 * nothing else; stats6 is added to as ur_object_id_pass adds to it, except [3], which is never touched (there is no queue).
 * UR_EINVAL, nothing launched: ur_gbuffer_pass' cases for the context, matrices, draws, depth, w, h, flags and key_triangle_bits;
 * point_count > UR_PICK_MAX_POINTS; with point_count != 0 a null points_xy, a null results or one not 16-byte aligned, results
 * overlapping depth or the commands.
 * UR_EUNSUPPORTED, nothing launched: key_triangle_bits == 0 with command_count >= 2^24. */
int ur_object_id_pick(ur_ctx* ctx, const float view[16], const float projection[16], const ur_raster_draws* draws,
                      const float* depth, uint32_t w, uint32_t h, uint32_t flags, uint32_t key_triangle_bits,
                      const uint32_t* points_xy, uint32_t point_count, ur_pick_result* results, uint32_t* stats6);

#ifdef __cplusplus
}
#endif
#endif /* UR_RASTER_H */
