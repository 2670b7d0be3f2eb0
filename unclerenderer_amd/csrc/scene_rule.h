// The scene rule, once, for the kernels (csrc/scene_build.hip) and the serial host build (csrc/scene_host.cpp):
// the row-vector products, the divide and the corner walk of csrc/scene.cpp (RendererUtils.cpp:402-440), the constants record of a
// draw (RendererUtils.cpp:1029-1088), its command slot (DeferredRenderer.cpp:3301-3366) and the scene box (RendererUtils.cpp:277-286,
// 533-540). No HIP in it beyond the function qualifiers: the plain host compiler builds it.
// All arithmetic is uncontracted fp32 (the units that include this are built with -ffp-contract=off).
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/ur_scene_build.h"

#if defined(__HIPCC__)
#define UR_SCENE_HD __host__ __device__ inline
#else
#define UR_SCENE_HD inline
#endif

namespace ur_scene {

constexpr uint32_t kConstantsBytes = 608u, kConstantsPieces = 38u; // sizeof(ur_scene_constants) in bytes and in 16-byte pieces
constexpr uint32_t kFactorPieces = 11u;                           // sizeof(ur_scene_material_factors) / 16
static_assert(sizeof(ur_scene_constants) == kConstantsBytes && sizeof(ur_scene_material_factors) == 16u * kFactorPieces, "record sizes");
static_assert(sizeof(ur_scene_node) == 144u && sizeof(ur_scene_mesh) == 32u && sizeof(ur_scene_draw) == 32u && sizeof(ur_scene_build_summary) == 48u, "record sizes");
static_assert(sizeof(ur_mesh_info) == 56u, "record sizes");

// Row-vector matrices (DirectXMath side): m[r][c]
struct RM { float m[4][4]; };

UR_SCENE_HD RM rm_mul(const RM& A, const RM& B)
{
    RM R{};
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) R.m[i][j] = ((A.m[i][0] * B.m[0][j] + A.m[i][1] * B.m[1][j]) + A.m[i][2] * B.m[2][j]) + A.m[i][3] * B.m[3][j];
    return R;
}
// XMVector3TransformCoord: the divide by w included
UR_SCENE_HD void transform_coord(const RM& M, const float p[3], float out[3])
{
    float r[4];
    for (int j = 0; j < 4; ++j) r[j] = ((p[0] * M.m[0][j] + p[1] * M.m[1][j]) + p[2] * M.m[2][j]) + M.m[3][j];
    for (int j = 0; j < 3; ++j) out[j] = r[j] / r[3];
}
UR_SCENE_HD float min_of(float a, float b) { return b < a ? b : a; } // std::min(a, b): a NaN in b is ignored, one in a stays
UR_SCENE_HD float max_of(float a, float b) { return a < b ? b : a; } // std::max(a, b)

constexpr float kFloatMax = 3.402823466e38f;

// What a draw gets from its node and its mesh
struct Placed {
    RM world;
    float bounds_min[3], bounds_max[3], center[3], radius;
};

UR_SCENE_HD Placed place(const ur_scene_node& n, const ur_mesh_info& info)
{
    RM NW, S{}, R{}, T{};
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) NW.m[r][c] = n.node_world[r * 4 + c];
    S.m[0][0] = n.scale[0]; S.m[1][1] = n.scale[1]; S.m[2][2] = n.scale[2]; S.m[3][3] = 1.0f;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) R.m[r][c] = n.rotation[r * 3 + c];
    R.m[3][3] = 1.0f;
    for (int i = 0; i < 4; ++i) T.m[i][i] = 1.0f;
    T.m[3][0] = n.translate[0]; T.m[3][1] = n.translate[1]; T.m[3][2] = n.translate[2];

    Placed out;
    out.world = rm_mul(rm_mul(rm_mul(NW, S), R), T);
    for (int a = 0; a < 3; ++a) { out.bounds_min[a] = kFloatMax; out.bounds_max[a] = -kFloatMax; }
    for (int corner = 0; corner < 8; ++corner) {
        const float p[3] = {(corner & 1) ? info.max[0] : info.min[0], (corner & 2) ? info.max[1] : info.min[1], (corner & 4) ? info.max[2] : info.min[2]};
        float w[3];
        transform_coord(out.world, p, w);
        for (int a = 0; a < 3; ++a) { out.bounds_min[a] = min_of(out.bounds_min[a], w[a]); out.bounds_max[a] = max_of(out.bounds_max[a], w[a]); }
    }
    float node_scale = 0.0f; // ComputeMaxScale over the node matrix columns (RendererUtils.cpp:288-295)
    for (int c = 0; c < 3; ++c) node_scale = max_of(node_scale, sqrtf((NW.m[0][c] * NW.m[0][c] + NW.m[1][c] * NW.m[1][c]) + NW.m[2][c] * NW.m[2][c]));
    transform_coord(out.world, info.center, out.center);
    out.radius = (info.radius * n.max_scale) * node_scale;
    return out;
}

UR_SCENE_HD bool draw_in_range(const ur_scene_draw& d, uint32_t node_count, uint32_t mesh_count, uint32_t material_count, uint32_t slot_count)
{
    return d.node < node_count && d.mesh < mesh_count && d.material < material_count && d.constants_slot < slot_count;
}

UR_SCENE_HD uint32_t float_bits(float f) { uint32_t b; __builtin_memcpy(&b, &f, 4); return b; }
UR_SCENE_HD float bits_float(uint32_t b) { float f; __builtin_memcpy(&f, &b, 4); return f; }

// The 16 words of a draw's command slot (FIndirectDrawCommand, RendererUtils.h:102-111)
UR_SCENE_HD void command_words(const ur_scene_mesh& mesh, const ur_scene_draw& d, uint64_t constants_address, uint32_t w[16])
{
    w[0] = (uint32_t)mesh.vertices; w[1] = (uint32_t)(mesh.vertices >> 32); w[2] = mesh.vertex_bytes; w[3] = mesh.stride;
    w[4] = (uint32_t)mesh.indices; w[5] = (uint32_t)(mesh.indices >> 32); w[6] = mesh.index_bytes; w[7] = mesh.index_format;
    w[8] = (uint32_t)constants_address; w[9] = (uint32_t)(constants_address >> 32); w[10] = d.index_count; w[11] = 1u;
    w[12] = d.index_start; w[13] = 0u; w[14] = d.constants_slot; w[15] = 0u;
}

// 16-byte piece `piece` (4 .. 37) of a draw's constants record: the template's `t`, with the per-draw fields taken from the material
// record's pieces `f` and the draw's ObjectId. (Pieces 0-3 are World.)
UR_SCENE_HD void constants_piece(uint32_t piece, const uint32_t t[4], const uint32_t* f /* 44 words */, uint32_t object_id, uint32_t out[4])
{
    out[0] = t[0]; out[1] = t[1]; out[2] = t[2]; out[3] = t[3];
    if (piece == 16u) { out[0] = f[0]; out[1] = f[1]; out[2] = f[2]; }                       // BaseColor (LightIntensity stays)
    else if (piece == 20u) { out[0] = f[4]; out[1] = f[5]; out[2] = f[6]; }                  // EmissiveFactor
    else if (piece == 26u) { out[0] = f[7]; out[1] = f[8]; out[2] = f[3]; out[3] = f[9]; }   // Metallic, Roughness, BaseColorAlpha, AlphaCutoff
    else if (piece == 27u) { out[0] = f[10]; }                                              // AlphaMode
    else if (piece >= 28u && piece < 36u) { const uint32_t* s = f + 12u + 4u * (piece - 28u); out[0] = s[0]; out[1] = s[1]; out[2] = s[2]; out[3] = s[3]; }
    else if (piece == 37u) { out[0] = object_id; }                                          // ObjectId
}

// --- the scene box: order-preserving integer images of the floats, -0 below +0 ---
UR_SCENE_HD uint32_t ordered_key(float f)
{
    const uint32_t b = float_bits(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
UR_SCENE_HD float key_value(uint32_t k) { return bits_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

struct Box { uint32_t lo[3], hi[3]; };
UR_SCENE_HD Box empty_box()
{
    const uint32_t lo = ordered_key(kFloatMax), hi = ordered_key(-kFloatMax);
    return {{lo, lo, lo}, {hi, hi, hi}};
}
UR_SCENE_HD void box_add(Box& b, const float center[3], float radius)
{
    for (int a = 0; a < 3; ++a) {
        const float lo = center[a] - radius, hi = center[a] + radius;
        if (lo == lo) { const uint32_t k = ordered_key(lo); b.lo[a] = k < b.lo[a] ? k : b.lo[a]; }
        if (hi == hi) { const uint32_t k = ordered_key(hi); b.hi[a] = k > b.hi[a] ? k : b.hi[a]; }
    }
}
UR_SCENE_HD void finish_summary(const Box& b, uint32_t draw_count, uint32_t skipped, ur_scene_build_summary& s)
{
    float e2 = 0.0f;
    for (int a = 0; a < 3; ++a) {
        s.scene_min[a] = key_value(b.lo[a]);
        s.scene_max[a] = key_value(b.hi[a]);
        s.scene_center[a] = 0.5f * (s.scene_min[a] + s.scene_max[a]);
        e2 += (s.scene_max[a] - s.scene_min[a]) * (s.scene_max[a] - s.scene_min[a]);
    }
    s.scene_radius = max_of(sqrtf(e2) * 0.5f, 1.0f);
    s.draw_count = draw_count;
    s.skipped_draws = skipped;
}

// --- host only: the checks ur_scene_build and ur_host_scene_build share; 0, or 1 with the text ---
inline int check_tables(const char* who, const ur_scene_build_tables* t, const ur_scene_constants* frame, const ur_scene_build_outputs* o, uint32_t flags, char* text,
                        size_t cap)
{
    if (!t || !frame || !o) { snprintf(text, cap, "%s: null tables, frame or outputs", who); return 1; }
    if (!t->nodes || !t->meshes || !t->mesh_infos || !t->materials || !t->draws) { snprintf(text, cap, "%s: null table", who); return 1; }
    if (!o->bounds || !o->commands || !o->constants || !o->summary) { snprintf(text, cap, "%s: null bounds, commands, constants or summary", who); return 1; }
    if (t->draw_count == 0u || t->draw_count >= UR_SCENE_BUILD_MAX_DRAWS) { snprintf(text, cap, "%s: %u draws (1 .. 2^24 - 1)", who, t->draw_count); return 1; }
    if (t->node_count == 0u || t->mesh_count == 0u || t->material_count == 0u) { snprintf(text, cap, "%s: an empty table (%u nodes, %u meshes, %u materials)", who, t->node_count, t->mesh_count, t->material_count); return 1; }
    if (o->slot_count == 0u) { snprintf(text, cap, "%s: no constants slots", who); return 1; }
    if (o->constants_stride < kConstantsBytes || o->constants_stride % 16u != 0u) { snprintf(text, cap, "%s: constants stride %u (at least 608, a multiple of 16)", who, o->constants_stride); return 1; }
    if (flags & ~UR_SCENE_BUILD_TRANSFORMS_ONLY) { snprintf(text, cap, "%s: unknown flag bits 0x%x", who, flags & ~UR_SCENE_BUILD_TRANSFORMS_ONLY); return 1; }
    return 0;
}

} // namespace ur_scene
