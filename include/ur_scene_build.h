/*
 * ur_scene_build.h - scene build: the meshes ur_mesh_build left on the device (include/ur_mesh.h) and tables of node transforms,
 * material factors and draws become what the cull and the raster passes take - the ModelBounds of ur_cull_indirect_args*, the
 * 64-byte FIndirectDrawCommand slots of include/ur_raster.h and one ur_scene_constants record per draw - in one asynchronous call, on
 * the device, with nothing read back. The reference does this on the host: CreateSceneModelsFromJson
 * (RendererUtils.cpp:298-543), CreateGpuDrivenResources (DeferredRenderer.cpp:3292-3472), UpdateSceneConstants
 * (RendererUtils.cpp:1029-1088). The same rule in plain serial C++ is ur_host_scene_build (include/ur_host.h).
 *
 * The rule per draw, in uncontracted fp32 as in csrc/scene.cpp (every product and every sum is rounded on its own):
 *   World   = ((node_world * Scale) * Rotation) * Translation, row-major, row vectors, every element a full four-term sum
 *   bounds  = min / max (std::min / std::max, from +-FLT_MAX) over the eight corners of the mesh's box through World, divided by w,
 *             corner c taking max.x when c & 1, max.y when c & 2, max.z when c & 4
 *   centre  = the mesh's centre through World, divided by w
 *   radius  = (mesh radius * max_scale) * the largest column length of node_world's upper 3 x 3
 * The scene box is over centre +- radius of the draws that are not skipped, from +-FLT_MAX, per axis the minimum and the maximum in the
 * total order in which a NaN is ignored and -0 lies below +0; then center = 0.5f * (min + max) and
 * radius = max(sqrt(sum of squared extents) * 0.5f, 1.0f). ur_scene_extract (include/ur_scene.h) folds the same values serially with
 * std::min / std::max, to which -0 and +0 are equal, so that of the two the first met stays: the two summaries differ in the sign of a
 * zero at most.
 */
#ifndef UR_SCENE_BUILD_H
#define UR_SCENE_BUILD_H

#include <stdint.h>

#include "ur_hotpath.h"
#include "ur_mesh.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ur_scene_build puts at most this many operations on the context's stream (today two: the build launch and the finish launch). */
#define UR_SCENE_BUILD_MAX_STREAM_OPS 3u
/* flags: write only bounds, centers, bytes 0-63 (World) of each named slot and the summary; commands and bytes 64-607 keep their bytes */
#define UR_SCENE_BUILD_TRANSFORMS_ONLY 0x1u
#define UR_SCENE_BUILD_MAX_DRAWS (1u << 24) /* draw_count is below this */

/* A node of a placed model: the glTF node's world matrix and the model's scale, rotation and translation. rotation is the upper 3 x 3
 * of XMMatrixRotationRollPitchYaw, row-major (the sines and cosines stay on the host); max_scale is max |scale[k]|. reserved is 0. */
typedef struct ur_scene_node {
    float node_world[16]; /* row-major, row vectors */
    float scale[3], max_scale;
    float rotation[9];
    float translate[3];
    uint32_t reserved[4];
} ur_scene_node; /* 144 bytes */

/* A built mesh: device addresses and sizes as a command slot carries them (words 0-7 of FIndirectDrawCommand). */
typedef struct ur_scene_mesh {
    uint64_t vertices, indices;
    uint32_t vertex_bytes, index_bytes, stride, index_format;
} ur_scene_mesh; /* 32 bytes */

/* The per-material fields of ur_scene_constants. transforms: BaseColorTransformOffsetScale ... EmissiveTransformRotation in
 * ur_scene_constants' order. */
typedef struct ur_scene_material_factors {
    float BaseColor[3], BaseColorAlpha;
    float EmissiveFactor[3], MetallicFactor;
    float RoughnessFactor, AlphaCutoff;
    uint32_t AlphaMode, Padding;
    float transforms[8][4];
} ur_scene_material_factors; /* 176 bytes */

/* One draw, in command order: indices into the three tables, the constants record it owns, the ObjectId it writes and its section of
 * the mesh's indices. Distinct draws name distinct slots: that is the caller's contract. reserved is 0. */
typedef struct ur_scene_draw {
    uint32_t node, mesh, material, constants_slot;
    uint32_t object_id, index_start, index_count, reserved;
} ur_scene_draw; /* 32 bytes */

typedef struct ur_scene_build_summary {
    float scene_min[3], scene_max[3], scene_center[3], scene_radius;
    uint32_t draw_count, skipped_draws;
} ur_scene_build_summary; /* 48 bytes */

/* The tables: device memory, 16-byte aligned, only read. mesh_infos: mesh_count records of 56 bytes each, as ur_mesh_build writes them
 * (it accepts any 4-byte aligned info pointer, so each build can write its own record of one array). */
typedef struct ur_scene_build_tables {
    const ur_scene_node* nodes;
    const ur_scene_mesh* meshes;
    const ur_mesh_info* mesh_infos;
    const ur_scene_material_factors* materials;
    const ur_scene_draw* draws;
    uint32_t node_count, mesh_count, material_count, draw_count;
} ur_scene_build_tables;

/* The outputs: device memory, 16-byte aligned. With D = draw_count:
 *   bounds     2 * D ur_float4: (min.xyz, 0)(max.xyz, 0), the ModelBounds of ur_cull_indirect_args*
 *   commands   D * 64 bytes: words 0-7 the mesh record's, 8-9 constants + slot * constants_stride, 10 index_count, 11 InstanceCount 1,
 *              12 index_start, 13 BaseVertex 0, 14 constants_slot (the reference's StartInstanceLocation), 15 zero
 *   constants  slot_count * constants_stride bytes; constants_stride >= 608 and a multiple of 16. Bytes 0-607 of a named slot are
 *              written, the bytes from 608 up to the stride are left alone, a slot no draw names is left alone
 *   centers    D ur_float4 (centre.xyz, radius), or NULL
 *   summary    one ur_scene_build_summary */
typedef struct ur_scene_build_outputs {
    ur_float4* bounds;
    void* commands;
    void* constants;
    ur_float4* centers;
    ur_scene_build_summary* summary;
    uint32_t constants_stride, slot_count;
} ur_scene_build_outputs;

/* Bytes of scratch a build of draw_count draws needs (a multiple of 16); 0 for draw_count == 0 or >= UR_SCENE_BUILD_MAX_DRAWS. */
uint64_t ur_scene_build_scratch_bytes(uint32_t draw_count);

/* Builds the scene on the context's stream: asynchronous, the host reads no device memory and does not synchronise; at most
 * UR_SCENE_BUILD_MAX_STREAM_OPS stream operations. `tables`, `frame` and `outputs` are host memory, read before the call returns.
 *
 * The constants record of a draw is *frame with these fields overwritten: World from the node; BaseColor, EmissiveFactor,
 * MetallicFactor, RoughnessFactor, BaseColorAlpha, AlphaCutoff, AlphaMode and the eight transforms from the draw's material record;
 * ObjectId from the draw.
 *
 * A draw whose node, mesh, material or constants_slot is out of range is skipped: its command and its two bounds are zero bytes, its
 * centers entry is zero, no slot is written, it adds nothing to the scene box and it counts in skipped_draws. (With
 * UR_SCENE_BUILD_TRANSFORMS_ONLY its command keeps its bytes like every other.)
 *
 * scratch: device memory, 16-byte aligned, scratch_bytes >= ur_scene_build_scratch_bytes(draw_count); the build writes every byte of it
 * that it reads, so what it holds on entry does not matter.
 *
 * UR_EINVAL (ur_last_error has the text), decided from the arguments alone, nothing launched: a null pointer (centers may be null) or
 * a misaligned one, draw_count == 0 or >= UR_SCENE_BUILD_MAX_DRAWS, an empty table, slot_count == 0, a stride below 608 or no multiple
 * of 16, unknown flag bits, too little scratch, outputs that overlap each other, the tables or the scratch. */
int ur_scene_build(ur_ctx* ctx, const ur_scene_build_tables* tables, const ur_scene_constants* frame, const ur_scene_build_outputs* outputs, void* scratch,
                   uint64_t scratch_bytes, uint32_t flags);

#ifdef __cplusplus
}
#endif
#endif /* UR_SCENE_BUILD_H */
