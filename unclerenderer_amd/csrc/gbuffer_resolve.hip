// GBuffer's resolve for gfx950 — a lane per texel of the band turns the winning visibility key (csrc/raster.hip) into the render
// targets: it fetches the key's triangle again, restates the near clip with a weight row per polygon vertex, interpolates the attributes
// perspective-correct and runs the base pass' pixel shader (Shaders/DeferredBasePass.hlsl), with or without ObjectId and texture maps
// (csrc/texture_sample.h). DESIGN.md sections 3.9 and 3.10 are its rule, tests/gbuffer_ref.py the restatement. Built with -ffp-contract=off.
// The entry points of the Forward pass sit here too: they share gbuffer_entry's checks and raster launches, and
// their resolve is csrc/forward_resolve.hip's.

#include "forward_resolve.h"
#include "gbuffer_interp.h"
#include "lighting_plan.h"
#include "raster_rule.h"
#include "resolve_pack.h"
#include "texture_sample.h"
#include "ur_device.h"
#include "ur_internal.h"

namespace {

using namespace ur_raster;

static_assert(sizeof(ur_texture2d) == 16 && sizeof(ur_material) == 80, "ur_material is 80 bytes");

struct ResolveParams {
    const uint8_t* commands;
    uint32_t mode; // 0 every slot / ranges (the ordinal is the slot), 1 list (the ordinal is the position in the list)
    const uint32_t* visible_idx;
    uint32_t index_base;
    float V[16], Pr[16];
    const uint32_t* keys;
    uint2* gbuf_a; uint2* gbuf_b; uint32_t* gbuf_c; uint2* hdr; uint32_t* object_id;
    const float* table; // 255 thresholds of the sRGB encode
    uint32_t w, row0, n;  // n = rows * w
    float half_w, half_h;
    uint32_t key_bits;
    // the textured resolve
    const ur_material* materials;
    uint32_t material_count;
    const float* decode; // 256 entries of the sRGB decode
    const float* lod;    // 127 thresholds of the level of detail
    // with masked draws under visible lists: a texel's key is a position in the masked list iff its word is not 0
    const unsigned long long* keys64;
    const uint32_t* mask_visible_idx;
    uint32_t mask_mode, mask_index_base;
};

// the number of thresholds with x >= entry (ascending entries: a binary search; every compare is false for a NaN: 0)
__device__ __forceinline__ uint32_t srgb_code(const float* table, float x)
{
    uint32_t lo = 0u, hi = 255u;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint32_t mid = (lo + hi) >> 1;
        const bool ge = lo < hi && x >= table[min(mid, 254u)];
        if (lo < hi) { if (ge) lo = mid + 1u; else hi = mid; }
    }
    return lo;
}

template <bool OBJECT_ID, bool MAPS = false, bool MASKED = false>
__global__ __launch_bounds__(kThreads) void gbuffer_resolve_kernel(ResolveParams p)
{
    __shared__ float table[256];
    __shared__ float sampler_tables[MAPS ? kLdsFloats : 1u];
    table[threadIdx.x] = p.table[min(threadIdx.x, 254u)];
    if constexpr (MAPS) {
        sampler_tables[kLdsDecode + threadIdx.x] = p.decode[threadIdx.x];
        sampler_tables[kLdsUnorm + threadIdx.x] = (float)threadIdx.x / 255.0f;
        if (threadIdx.x < 128u) sampler_tables[kLdsLod + threadIdx.x] = p.lod[min(threadIdx.x, 126u)];
    }
    __syncthreads();
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= p.n) return;
    const uint32_t key = p.keys[i];
    if (key == 0u) { // the clear values
        const ur::once_u32x2_t clear = {0u, 0x3C000000u}; // fp16 (0, 0, 0, 1)
        ur::store_once_b64(p.gbuf_a + i, clear);
        ur::store_once_b64(p.gbuf_b + i, clear);
        ur::store_once_b32(p.gbuf_c + i, 0xFF000000u);
        ur::store_once_b64(p.hdr + i, clear);
        if constexpr (OBJECT_ID) ur::store_once_b32(p.object_id + i, 0u);
        return;
    }
    const uint32_t ordinal = (key >> p.key_bits) - 1u, t = key & ((1u << p.key_bits) - 1u);
    uint32_t slot = p.mode == 1u ? p.visible_idx[ordinal] - p.index_base : ordinal;
    if constexpr (MASKED) {
        if (p.keys64[i] != 0ull) slot = p.mask_mode == 1u ? p.mask_visible_idx[ordinal] - p.mask_index_base : ordinal;
    }
    const u32x4_t* cmd = reinterpret_cast<const u32x4_t*>(p.commands + (size_t)slot * UR_INDIRECT_COMMAND_STRIDE);
    const u32x4_t c0 = cmd[0], c1 = cmd[1], c2 = cmd[2], c3 = cmd[3];
    const uint8_t* vertices = reinterpret_cast<const uint8_t*>((uint64_t)c0.x | ((uint64_t)c0.y << 32));
    const uint32_t* indices = reinterpret_cast<const uint32_t*>((uint64_t)c1.x | ((uint64_t)c1.y << 32));
    const float* cb = reinterpret_cast<const float*>((uint64_t)c2.x | ((uint64_t)c2.y << 32));
    const uint32_t stride = c0.w;
    const uint64_t first = (uint64_t)c3.x + 3ull * t;
    const long long base_vertex = (int)c3.y;
    float W[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) W[k] = cb[k];

    // ---- the three vertices: rule 1 (world and clip position), the world normal, the colour
    float c[3][4], wp[3][3], wn[3][3], col[3][3];
    [[maybe_unused]] float uv[3][2], tg[3][4]; // MAPS: TEXCOORD and the vertex shader's tangent
#pragma unroll
    for (int v = 0; v < 3; ++v) {
        const uint64_t vi = (uint64_t)(base_vertex + (long long)indices[first + (uint32_t)v]);
        const f32x4u_t* vp = reinterpret_cast<const f32x4u_t*>(vertices + vi * stride);
        const f32x4u_t v0 = vp[0], v1 = vp[1], v3 = vp[3];
        const float x = v0.x, y = v0.y, z = v0.z, nx = v0.w, ny = v1.x, nz = v1.y;
        float wv[4], vv[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) wv[k] = ((x * W[k] + y * W[4 + k]) + z * W[8 + k]) + W[12 + k];
#pragma unroll
        for (int k = 0; k < 4; ++k) vv[k] = ((wv[0] * p.V[k] + wv[1] * p.V[4 + k]) + wv[2] * p.V[8 + k]) + wv[3] * p.V[12 + k];
#pragma unroll
        for (int k = 0; k < 4; ++k) c[v][k] = ((vv[0] * p.Pr[k] + vv[1] * p.Pr[4 + k]) + vv[2] * p.Pr[8 + k]) + vv[3] * p.Pr[12 + k];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            wp[v][k] = wv[k];
            wn[v][k] = (nx * W[k] + ny * W[4 + k]) + nz * W[8 + k];
        }
        col[v][0] = v3.x; col[v][1] = v3.y; col[v][2] = v3.z;
        if constexpr (MAPS) {
            const f32x4u_t v2 = vp[2];
            uv[v][0] = v1.z; uv[v][1] = v1.w;
            float wt[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) wt[k] = (v2.x * W[k] + v2.y * W[4 + k]) + v2.z * W[8 + k];
            const float tl = sqrtf((wt[0] * wt[0] + wt[1] * wt[1]) + wt[2] * wt[2]);
            tg[v][0] = wt[0] / tl; tg[v][1] = wt[1] / tl; tg[v][2] = wt[2] / tl; tg[v][3] = v2.w;
        }
    }

    // ---- rule 2 again with a weight row per polygon vertex, the piece that covers this centre and its weights (gbuffer_interp.h)
    float SX[4], SY[4], vw[4], B[4][3];
    bool one;
    clip_polygon(c, p.half_w, p.half_h, SX, SY, vw, B, one);
    const uint32_t row = i / p.w, column = i - row * p.w;
    Piece pc;
    covering_piece(SX, SY, vw, one, 256 * (int)column + 128, 256 * (int)(p.row0 + row) + 128, pc);
    float b[3];
    piece_weights(pc, pc.l0, pc.l1, pc.l2, B, b);
    float n[3], wpos[3], colour[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        n[k] = (b[0] * wn[0][k] + b[1] * wn[1][k]) + b[2] * wn[2][k];
        wpos[k] = (b[0] * wp[0][k] + b[1] * wp[1][k]) + b[2] * wp[2][k];
        colour[k] = (b[0] * col[0][k] + b[1] * col[1][k]) + b[2] * col[2][k];
    }

    if constexpr (MAPS) {
        // ---- the material of the slot, its valid maps, and the samples
        uint32_t bits = 0u;
        if (slot < p.material_count) bits = reinterpret_cast<const uint32_t*>(p.materials + slot)[16] & 15u;
        float base[3] = {1.0f, 1.0f, 1.0f}, mr[3] = {1.0f, 1.0f, 1.0f}, nm[3] = {0.5f, 0.5f, 1.0f}, em[3] = {1.0f, 1.0f, 1.0f};
        if (__ballot(bits != 0u) != 0ull) {
            const bool odd_column = (column & 1u) != 0u, odd_row = ((p.row0 + row) & 1u) != 0u;
            float pu[3], pv[3]; // TEXCOORD at the centre, the horizontal and the vertical partner
            quad_texcoords(pc, B, uv, odd_column, odd_row, pu, pv);
#pragma unroll 1
            for (uint32_t map = 0u; map < 4u; ++map) { // t0 base colour, t1 metallic-roughness, t2 normal, t3 emissive
                const uint32_t bit = map == 0u ? UR_MATERIAL_BASE_COLOR_MAP : (map == 1u ? UR_MATERIAL_METALLIC_ROUGHNESS_MAP : (map == 2u ? UR_MATERIAL_NORMAL_MAP : UR_MATERIAL_EMISSIVE_MAP));
                if (__ballot((bits & bit) != 0u) == 0ull) continue;
                if ((bits & bit) == 0u) continue;
                const u32x4_t desc = reinterpret_cast<const u32x4_t*>(p.materials + slot)[map];
                if (!valid_texture(desc)) { bits &= ~bit; continue; }
                const uint32_t at = 112u + 8u * map; // the map's OffsetScale and Rotation in ur_scene_constants
                float tu[3], tv[3];
#pragma unroll
                for (int point = 0; point < 3; ++point) texture_transform(cb, at, pu[point], pv[point], tu[point], tv[point]);
                // value(odd) - value(even)
                const float dxu = odd_column ? tu[0] - tu[1] : tu[1] - tu[0], dxv = odd_column ? tv[0] - tv[1] : tv[1] - tv[0];
                const float dyu = odd_row ? tu[0] - tu[2] : tu[2] - tu[0], dyv = odd_row ? tv[0] - tv[2] : tv[2] - tv[0];
                float s[3];
                sample_map(desc, tu[0], tv[0], dxu, dxv, dyu, dyv, sampler_tables, s);
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    if (map == 0u) base[k] = s[k];
                    if (map == 1u) mr[k] = s[k];
                    if (map == 2u) nm[k] = s[k];
                    if (map == 3u) em[k] = s[k];
                }
            }
        }
        // ---- the pixel shader (DeferredBasePass.hlsl:80-148)
        const float nl = sqrtf((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
        const float vn[3] = {n[0] / nl, n[1] / nl, n[2] / nl};
        float wnrm[3] = {vn[0], vn[1], vn[2]};
        if (bits & UR_MATERIAL_NORMAL_MAP) {
            float tan4[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) tan4[k] = (b[0] * tg[0][k] + b[1] * tg[1][k]) + b[2] * tg[2][k];
            const float dt = (vn[0] * tan4[0] + vn[1] * tan4[1]) + vn[2] * tan4[2];
            const float u0 = tan4[0] - vn[0] * dt, u1 = tan4[1] - vn[1] * dt, u2 = tan4[2] - vn[2] * dt;
            const float ul = sqrtf((u0 * u0 + u1 * u1) + u2 * u2);
            const float t0 = u0 / ul, t1 = u1 / ul, t2 = u2 / ul;
            const float c0 = vn[1] * t2 - vn[2] * t1, c1 = vn[2] * t0 - vn[0] * t2, c2 = vn[0] * t1 - vn[1] * t0;
            const float cl = sqrtf((c0 * c0 + c1 * c1) + c2 * c2);
            const float bt0 = (c0 / cl) * tan4[3], bt1 = (c1 / cl) * tan4[3], bt2 = (c2 / cl) * tan4[3];
            const float nr = nm[0] * 2.0f - 1.0f, ng = nm[1] * 2.0f - 1.0f;
            const float one_minus = 1.0f - (nr * nr + ng * ng);
            const float nz = sqrtf(one_minus > 0.0f ? fminf(one_minus, 1.0f) : 0.0f); // saturate
            const float tl = sqrtf((nr * nr + ng * ng) + nz * nz);
            const bool flat = tl < 1e-5f;
            const float e0 = flat ? 0.0f : nr, e1 = flat ? 0.0f : ng, e2 = flat ? 1.0f : nz;
            const float w0 = (e0 * t0 + e1 * bt0) + e2 * vn[0], w1 = (e0 * t1 + e1 * bt1) + e2 * vn[1], w2 = (e0 * t2 + e1 * bt2) + e2 * vn[2];
            const float wl = sqrtf((w0 * w0 + w1 * w1) + w2 * w2);
            wnrm[0] = w0 / wl; wnrm[1] = w1 / wl; wnrm[2] = w2 / wl;
        }
        float m[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) m[k] = (wnrm[0] * p.V[k] + wnrm[1] * p.V[4 + k]) + wnrm[2] * p.V[8 + k];
        const float ml = sqrtf((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
        const float view_depth = -(((wpos[0] * p.V[2] + wpos[1] * p.V[6]) + wpos[2] * p.V[10]) + p.V[14]);
        float albedo[3] = {cb[64] * colour[0], cb[65] * colour[1], cb[66] * colour[2]};
        float metallic = cb[104], roughness = cb[105];
        float emissive[3] = {cb[80], cb[81], cb[82]};
        if (bits & UR_MATERIAL_BASE_COLOR_MAP) { albedo[0] = albedo[0] * base[0]; albedo[1] = albedo[1] * base[1]; albedo[2] = albedo[2] * base[2]; }
        if (bits & UR_MATERIAL_METALLIC_ROUGHNESS_MAP) { metallic = metallic * mr[2]; roughness = roughness * mr[1]; }
        if (bits & UR_MATERIAL_EMISSIVE_MAP) { emissive[0] = emissive[0] * em[0]; emissive[1] = emissive[1] * em[1]; emissive[2] = emissive[2] * em[2]; }
        const uint32_t r8 = srgb_code(table, albedo[0]), g8 = srgb_code(table, albedo[1]), b8 = srgb_code(table, albedo[2]);
        ur::store_once_b64(p.gbuf_a + i, pack_half4(m[0] / ml, m[1] / ml, m[2] / ml, view_depth));
        ur::store_once_b64(p.gbuf_b + i, pack_half4(0.04f, metallic, roughness, 1.0f));
        ur::store_once_b32(p.gbuf_c + i, r8 | (g8 << 8) | (b8 << 16) | 0xFF000000u);
        ur::store_once_b64(p.hdr + i, pack_half4(emissive[0], emissive[1], emissive[2], 1.0f));
        if constexpr (OBJECT_ID) ur::store_once_b32(p.object_id + i, reinterpret_cast<const uint32_t*>(cb)[148]);
        return;
    }

    // ---- the pixel shader (DeferredBasePass.hlsl:80-149 without maps)
    const float nl = sqrtf((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
    const float vn0 = n[0] / nl, vn1 = n[1] / nl, vn2 = n[2] / nl;
    float m[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) m[k] = (vn0 * p.V[k] + vn1 * p.V[4 + k]) + vn2 * p.V[8 + k];
    const float ml = sqrtf((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
    const float view_depth = -(((wpos[0] * p.V[2] + wpos[1] * p.V[6]) + wpos[2] * p.V[10]) + p.V[14]);
    const uint32_t r8 = srgb_code(table, cb[64] * colour[0]), g8 = srgb_code(table, cb[65] * colour[1]), b8 = srgb_code(table, cb[66] * colour[2]);
    ur::store_once_b64(p.gbuf_a + i, pack_half4(m[0] / ml, m[1] / ml, m[2] / ml, view_depth));
    ur::store_once_b64(p.gbuf_b + i, pack_half4(0.04f, cb[104], cb[105], 1.0f));
    ur::store_once_b32(p.gbuf_c + i, r8 | (g8 << 8) | (b8 << 16) | 0xFF000000u);
    ur::store_once_b64(p.hdr + i, pack_half4(cb[80], cb[81], cb[82], 1.0f));
    if constexpr (OBJECT_ID) ur::store_once_b32(p.object_id + i, reinterpret_cast<const uint32_t*>(cb)[148]);
}

// What ur_forward_pass adds to a GBuffer call: its targets are hdr and keys alone, and the resolve shades (csrc/forward_resolve.hip)
struct ForwardCall {
    const ur_scene_constants* frame;
    const ur_lighting_tables* tables;
};

// ur_forward_pass' own checks (the draws, depth and the matrices have passed theirs); fills in the staged cube's layout
int check_forward_call(const char* who, const ForwardCall& f, const ur_gbuffer_targets* targets, const ur_raster_draws& draws, const float* depth,
                       const ur_material* materials, uint32_t material_count, uint32_t w, uint32_t h, uint32_t rows, ur::CubeLayout& cube)
{
    if (!targets || !targets->hdr || !targets->keys) { ur::set_error("%s: null targets, hdr or keys", who); return UR_EINVAL; }
    if (!aligned(targets->hdr, 8) || !aligned(targets->keys, 4)) { ur::set_error("%s: a misaligned target (hdr 8 bytes, keys 4)", who); return UR_EINVAL; }
    if (!f.frame || !f.tables) { ur::set_error("%s: null frame_constants or tables", who); return UR_EINVAL; }
    const ur_lighting_tables& t = *f.tables;
    const float sw = f.frame->ShadowMapSize[0], sh = f.frame->ShadowMapSize[1];
    const bool shadows = f.frame->ShadowStrength > 0.0f;
    if (shadows && (!t.shadow_map || !(sw >= 1.0f && sw <= (float)UR_RASTER_MAX_TARGET) || !(sh >= 1.0f && sh <= (float)UR_RASTER_MAX_TARGET))) {
        ur::set_error("%s: ShadowStrength > 0 without a shadow map, or a ShadowMapSize outside 1..%u", who, UR_RASTER_MAX_TARGET);
        return UR_EINVAL;
    }
    if (!t.env_cube || t.env_base_size == 0u || t.env_mip_count == 0u || t.env_mip_count > 16u || !t.brdf_lut_rg16 || t.lut_width == 0u || t.lut_height == 0u ||
        !aligned(t.env_cube, 8) || !aligned(t.brdf_lut_rg16, 4) || !aligned(t.shadow_map, 4)) {
        ur::set_error("%s: bad lighting tables (a null or misaligned cube or LUT, a zero size, no mip or more than 16)", who);
        return UR_EINVAL;
    }
    cube = ur::cube_layout(t.env_base_size, t.env_mip_count);
    if (cube.mips == 0u || t.env_cube_texels != cube.texels) {
        ur::set_error("%s: ur_lighting_tables.env_cube_texels = %llu, but ur_stage_env_cube writes %llu texels for a %u^2 cube of %u mips", who,
                      (unsigned long long)t.env_cube_texels, (unsigned long long)cube.texels, t.env_base_size, t.env_mip_count);
        return UR_EINVAL;
    }
    const size_t n = (size_t)w * rows;
    const struct { const void* at; size_t bytes; } inputs[] = {
        {depth, (size_t)w * h * 4u}, {ur::raster_commands(draws), (size_t)draws.command_count * UR_INDIRECT_COMMAND_STRIDE},
        {materials, (size_t)material_count * sizeof(ur_material)}, {shadows ? t.shadow_map : nullptr, (size_t)sw * (size_t)sh * 4u},
        {t.env_cube, (size_t)cube.texels * 8u}, {t.brdf_lut_rg16, (size_t)t.lut_width * t.lut_height * 4u}};
    for (const auto& in : inputs) {
        if (in.at && in.bytes && (ur::overlaps(targets->hdr, n * 8u, in.at, in.bytes) || ur::overlaps(targets->keys, n * 4u, in.at, in.bytes))) {
            ur::set_error("%s: hdr or keys overlaps an input (depth, the commands, the materials or a lighting table)", who);
            return UR_EINVAL;
        }
    }
    if (ur::overlaps(targets->hdr, n * 8u, targets->keys, n * 4u)) { ur::set_error("%s: hdr overlaps keys", who); return UR_EINVAL; }
    return UR_OK;
}

// The checks and the launches behind the GBuffer and the Forward entry points; `who` names the caller in the error text, `who_parts` its
// _parts form; `forward`: ur_forward_pass (targets then holds hdr and keys alone)
int gbuffer_entry(const char* who, const char* who_parts, ur_ctx* ctx, const float* view, const float* projection, const ur_raster_draws* draws, const float* depth,
                  const ur_gbuffer_targets* targets, uint32_t w, uint32_t h, uint32_t row0, uint32_t rows, uint32_t flags, uint32_t key_triangle_bits,
                  uint32_t* stats6, uint32_t parts, const ur_material* materials, uint32_t material_count, const ur_gbuffer_mask* mask = nullptr,
                  float* depth_out = nullptr, const ForwardCall* forward = nullptr)
{
    ur::CubeLayout cube{};
    int rc = ur::check_raster_call(who, ctx, view, projection, draws, depth, "depth", w, h, stats6);
    if (rc == UR_OK) rc = ur::check_depth_flags(who, flags);
    if (rc == UR_OK && !forward) rc = ur::check_gbuffer_targets(who, targets);
    if (rc == UR_OK) rc = ur::check_key_triangle_bits(who, key_triangle_bits);
    if (rc != UR_OK) return rc;
    if (rows == 0u || (uint64_t)row0 + rows > h) { ur::set_error("%s: rows [%u, %u + %u) of a target %u high", who, row0, row0, rows, h); return UR_EINVAL; }
    if (parts == 0u || (parts & ~(UR_GBUFFER_PART_RASTER | UR_GBUFFER_PART_RESOLVE))) { ur::set_error("%s: parts 0x%x (UR_GBUFFER_PART_RASTER | UR_GBUFFER_PART_RESOLVE)", who_parts, parts); return UR_EINVAL; }
    uint32_t key_bits = key_triangle_bits;
    if (key_bits == 0u) {
        if (draws->command_count >= (1u << 24)) {
            ur::set_error("%s: %u command slots leave fewer than 8 key bits for the triangle: pass key_triangle_bits", who, draws->command_count);
            return UR_EUNSUPPORTED;
        }
        uint32_t length = 0u;
        while ((draws->command_count >> length) != 0u) ++length;
        key_bits = min(32u - length, 31u);
    } else if ((uint64_t)draws->command_count >= (1ull << (32u - key_bits))) {
        ur::set_error("%s: %u command slots do not fit the %u key bits beside key_triangle_bits %u", who, draws->command_count, 32u - key_bits, key_bits);
        return UR_EINVAL;
    }
    if (!aligned(materials, 16)) { ur::set_error("%s: a misaligned material table (16 bytes)", who); return UR_EINVAL; }
    if (forward) {
        rc = check_forward_call(who, *forward, targets, *draws, depth, materials, material_count, w, h, rows, cube);
        if (rc != UR_OK) return rc;
    }
    if (mask) {
        rc = ur::check_gbuffer_mask(who, *draws, *mask, *targets, depth, w, h, rows);
        if (rc != UR_OK) return rc;
    }
    // ---- the launches: the raster over the key image (UR_GBUFFER_PART_RASTER), then the resolve (UR_GBUFFER_PART_RESOLVE)
    const uint32_t n = w * rows;
    if (parts & UR_GBUFFER_PART_RASTER) {
        rc = ur::launch_visibility_raster(ctx, view, projection, draws, depth, targets->keys, w, h, row0, rows, key_bits, (flags & UR_DEPTH_QUANTIZE_D24) != 0u, stats6);
        if (rc != UR_OK) return rc;
        if (mask) {
            rc = ur::launch_masked_raster(ctx, view, projection, mask->draws, depth_out, mask->keys64, targets->keys, w, h, row0, rows, key_bits,
                                          (flags & UR_DEPTH_QUANTIZE_D24) != 0u, mask->stats6, materials, material_count, mask->won);
            if (rc != UR_OK) return rc;
        }
    }
    if (!(parts & UR_GBUFFER_PART_RESOLVE)) return UR_OK;
    if (forward) {
        ur::ForwardParams f{};
        f.commands = static_cast<const uint8_t*>(ur::raster_commands(*draws));
        f.mode = draws->visible_idx != nullptr ? 1u : 0u;
        f.visible_idx = draws->visible_idx; f.index_base = draws->index_base;
        for (int k = 0; k < 16; ++k) { f.V[k] = view[k]; f.Pr[k] = projection[k]; f.lvp[k] = forward->frame->LightViewProjection[k]; }
        f.keys = targets->keys; f.hdr = reinterpret_cast<uint2*>(targets->hdr);
        f.w = w; f.row0 = row0; f.n = n;
        f.half_w = 0.5f * (float)w; f.half_h = 0.5f * (float)h;
        f.key_bits = key_bits;
        f.materials = materials; f.material_count = material_count;
        f.decode = ctx->srgb_table; f.lod = ctx->lod_table;
        const bool lists = mask && (draws->visible_idx != nullptr || mask->draws->visible_idx != nullptr);
        if (lists) {
            f.keys64 = reinterpret_cast<const unsigned long long*>(mask->keys64);
            f.mask_mode = mask->draws->visible_idx != nullptr ? 1u : 0u;
            f.mask_visible_idx = mask->draws->visible_idx; f.mask_index_base = mask->draws->index_base;
        }
        const ur_scene_constants& S = *forward->frame;
        const ur_lighting_tables& T = *forward->tables;
        for (int k = 0; k < 3; ++k) { f.camera[k] = S.CameraPosition[k]; f.light_direction[k] = S.LightDirection[k]; f.light_color[k] = S.LightColor[k]; }
        f.light_intensity = S.LightIntensity;
        f.shadow_strength = S.ShadowStrength; f.shadow_bias = S.ShadowBias;
        f.shadow_size[0] = S.ShadowMapSize[0]; f.shadow_size[1] = S.ShadowMapSize[1];
        const float above = S.EnvMapMipCount - 1.0f;
        f.max_mip = above > 0.0f ? above : 0.0f;
        f.shadow = T.shadow_map;
        f.shadow_w = S.ShadowStrength > 0.0f ? (int)S.ShadowMapSize[0] : 0; f.shadow_h = S.ShadowStrength > 0.0f ? (int)S.ShadowMapSize[1] : 0;
        f.env = reinterpret_cast<const uint2*>(T.env_cube);
        f.env_base = T.env_base_size; f.env_mips = T.env_mip_count;
        for (uint32_t m = 0; m < 16u; ++m) f.env_offset[m] = m < T.env_mip_count ? (uint32_t)cube.bordered[m] : 0u;
        f.lut = reinterpret_cast<const uint32_t*>(T.brdf_lut_rg16);
        f.lut_w = T.lut_width; f.lut_h = T.lut_height;
        return ur::launch_forward_resolve(ctx, f, materials != nullptr, lists);
    }
    ResolveParams r{};
    r.commands = static_cast<const uint8_t*>(ur::raster_commands(*draws));
    r.mode = draws->visible_idx != nullptr ? 1u : 0u;
    r.visible_idx = draws->visible_idx; r.index_base = draws->index_base;
    for (int k = 0; k < 16; ++k) { r.V[k] = view[k]; r.Pr[k] = projection[k]; }
    r.keys = targets->keys;
    r.gbuf_a = reinterpret_cast<uint2*>(targets->gbuf_a); r.gbuf_b = reinterpret_cast<uint2*>(targets->gbuf_b); r.gbuf_c = targets->gbuf_c;
    r.hdr = reinterpret_cast<uint2*>(targets->hdr); r.object_id = targets->object_id;
    r.table = ctx->srgb_encode_table;
    r.w = w; r.row0 = row0; r.n = n;
    r.half_w = 0.5f * (float)w; r.half_h = 0.5f * (float)h;
    r.key_bits = key_bits;
    const uint32_t blocks = (n + kThreads - 1u) / kThreads;
    if (mask && (draws->visible_idx != nullptr || mask->draws->visible_idx != nullptr)) {
        // an ordinal is a position in its own selection's list: the resolve that looks at keys64 (no ObjectId beside a mask)
        r.keys64 = reinterpret_cast<const unsigned long long*>(mask->keys64);
        r.mask_mode = mask->draws->visible_idx != nullptr ? 1u : 0u;
        r.mask_visible_idx = mask->draws->visible_idx; r.mask_index_base = mask->draws->index_base;
        r.materials = materials; r.material_count = material_count;
        r.decode = ctx->srgb_table; r.lod = ctx->lod_table;
        if (materials) hipLaunchKernelGGL((gbuffer_resolve_kernel<false, true, true>), dim3(blocks), dim3(kThreads), 0, ctx->stream, r);
        else hipLaunchKernelGGL((gbuffer_resolve_kernel<false, false, true>), dim3(blocks), dim3(kThreads), 0, ctx->stream, r);
        UR_HIP_TRY(hipGetLastError());
        return UR_OK;
    }
    if (materials) { // the textured resolve
        r.materials = materials; r.material_count = material_count;
        r.decode = ctx->srgb_table; r.lod = ctx->lod_table;
        if (targets->object_id) hipLaunchKernelGGL((gbuffer_resolve_kernel<true, true>), dim3(blocks), dim3(kThreads), 0, ctx->stream, r);
        else hipLaunchKernelGGL((gbuffer_resolve_kernel<false, true>), dim3(blocks), dim3(kThreads), 0, ctx->stream, r);
        UR_HIP_TRY(hipGetLastError());
        return UR_OK;
    }
    if (targets->object_id) hipLaunchKernelGGL(gbuffer_resolve_kernel<true>, dim3(blocks), dim3(kThreads), 0, ctx->stream, r);
    else hipLaunchKernelGGL(gbuffer_resolve_kernel<false>, dim3(blocks), dim3(kThreads), 0, ctx->stream, r);
    UR_HIP_TRY(hipGetLastError());
    return UR_OK;
}

} // namespace

int ur::check_gbuffer_targets(const char* who, const ur_gbuffer_targets* targets)
{
    if (!targets || !targets->gbuf_a || !targets->gbuf_b || !targets->gbuf_c || !targets->hdr || !targets->keys) {
        ur::set_error("%s: null targets, or a null target other than object_id", who);
        return UR_EINVAL;
    }
    if (!aligned(targets->gbuf_a, 8) || !aligned(targets->gbuf_b, 8) || !aligned(targets->hdr, 8) || !aligned(targets->gbuf_c, 4) || !aligned(targets->object_id, 4) ||
        !aligned(targets->keys, 4)) {
        ur::set_error("%s: a misaligned target (gbuf_a, gbuf_b, hdr 8 bytes, the others 4)", who);
        return UR_EINVAL;
    }
    return UR_OK;
}

// The checks ur_gbuffer_pass_masked adds; the opaque draws, the targets and depth have passed theirs
int ur::check_gbuffer_mask(const char* who, const ur_raster_draws& draws, const ur_gbuffer_mask& mask, const ur_gbuffer_targets& targets, const float* depth, uint32_t w,
                           uint32_t h, uint32_t rows)
{
    if (!mask.draws) { set_error("%s: a mask without draws", who); return UR_EINVAL; }
    const int rc = check_raster_draws(who, *mask.draws, depth, "depth", mask.stats6);
    if (rc != UR_OK) return rc;
    if (raster_commands(*mask.draws) != raster_commands(draws) || mask.draws->command_count != draws.command_count) {
        set_error("%s: the masked draws select from other commands, or another command_count, than the opaque draws: their keys would not share one space", who);
        return UR_EINVAL;
    }
    if (!mask.keys64 || !aligned(mask.keys64, 8) || !aligned(mask.won, 4)) { set_error("%s: a null or misaligned keys64 (8 bytes) or a misaligned won (4 bytes)", who); return UR_EINVAL; }
    const size_t n = (size_t)w * rows;
    const struct { const void* at; size_t bytes; } others[] = {{targets.gbuf_a, n * 8u}, {targets.gbuf_b, n * 8u}, {targets.gbuf_c, n * 4u}, {targets.hdr, n * 8u},
                                                               {targets.keys, n * 4u}, {targets.object_id, n * 4u}, {depth, (size_t)w * h * 4u}};
    for (const auto& o : others) {
        if (o.at && overlaps(mask.keys64, n * 8u, o.at, o.bytes)) { set_error("%s: keys64 overlaps a target or depth", who); return UR_EINVAL; }
    }
    if (targets.object_id) {
        set_error("%s: object_id beside a mask: the ObjectId pass ignores the alpha test and tests against the depth this pass writes; it needs a raster of its own", who);
        return UR_EUNSUPPORTED;
    }
    return UR_OK;
}

extern "C" {

int ur_forward_pass_parts(ur_ctx* ctx, const float* view, const float* projection, const ur_raster_draws* draws, float* depth, const ur_forward_targets* targets,
                          uint32_t w, uint32_t h, uint32_t row0, uint32_t rows, uint32_t flags, uint32_t key_triangle_bits, uint32_t* stats6, uint32_t parts,
                          const ur_material* materials, uint32_t material_count, const ur_gbuffer_mask* mask, const ur_scene_constants* frame_constants,
                          const ur_lighting_tables* tables)
{
    ur_gbuffer_targets t{};
    if (targets) { t.hdr = targets->hdr; t.keys = targets->keys; }
    const ForwardCall forward{frame_constants, tables};
    return gbuffer_entry("ur_forward_pass", "ur_forward_pass_parts", ctx, view, projection, draws, depth, targets ? &t : nullptr, w, h, row0, rows, flags,
                         key_triangle_bits, stats6, parts, materials, material_count, mask, depth, &forward);
}

int ur_forward_pass(ur_ctx* ctx, const float* view, const float* projection, const ur_raster_draws* draws, float* depth, const ur_forward_targets* targets, uint32_t w,
                    uint32_t h, uint32_t row0, uint32_t rows, uint32_t flags, uint32_t key_triangle_bits, uint32_t* stats6, const ur_material* materials,
                    uint32_t material_count, const ur_gbuffer_mask* mask, const ur_scene_constants* frame_constants, const ur_lighting_tables* tables)
{
    return ur_forward_pass_parts(ctx, view, projection, draws, depth, targets, w, h, row0, rows, flags, key_triangle_bits, stats6,
                                 UR_GBUFFER_PART_RASTER | UR_GBUFFER_PART_RESOLVE, materials, material_count, mask, frame_constants, tables);
}

int ur_gbuffer_pass_masked_parts(ur_ctx* ctx, const float* view, const float* projection, const ur_raster_draws* draws, float* depth, const ur_gbuffer_targets* targets,
                                 uint32_t w, uint32_t h, uint32_t row0, uint32_t rows, uint32_t flags, uint32_t key_triangle_bits, uint32_t* stats6, uint32_t parts,
                                 const ur_material* materials, uint32_t material_count, const ur_gbuffer_mask* mask)
{
    return gbuffer_entry("ur_gbuffer_pass_masked", "ur_gbuffer_pass_masked_parts", ctx, view, projection, draws, depth, targets, w, h, row0, rows, flags, key_triangle_bits,
                         stats6, parts, materials, material_count, mask, depth);
}

int ur_gbuffer_pass_masked(ur_ctx* ctx, const float* view, const float* projection, const ur_raster_draws* draws, float* depth, const ur_gbuffer_targets* targets,
                           uint32_t w, uint32_t h, uint32_t row0, uint32_t rows, uint32_t flags, uint32_t key_triangle_bits, uint32_t* stats6,
                           const ur_material* materials, uint32_t material_count, const ur_gbuffer_mask* mask)
{
    return gbuffer_entry("ur_gbuffer_pass_masked", "ur_gbuffer_pass_masked_parts", ctx, view, projection, draws, depth, targets, w, h, row0, rows, flags, key_triangle_bits,
                         stats6, UR_GBUFFER_PART_RASTER | UR_GBUFFER_PART_RESOLVE, materials, material_count, mask, depth);
}

int ur_gbuffer_pass_materials_parts(ur_ctx* ctx, const float* view, const float* projection, const ur_raster_draws* draws, const float* depth,
                                    const ur_gbuffer_targets* targets, uint32_t w, uint32_t h, uint32_t row0, uint32_t rows, uint32_t flags, uint32_t key_triangle_bits,
                                    uint32_t* stats6, uint32_t parts, const ur_material* materials, uint32_t material_count)
{
    return gbuffer_entry("ur_gbuffer_pass_materials", "ur_gbuffer_pass_materials_parts", ctx, view, projection, draws, depth, targets, w, h, row0, rows, flags,
                         key_triangle_bits, stats6, parts, materials, material_count);
}

int ur_gbuffer_pass_materials(ur_ctx* ctx, const float* view, const float* projection, const ur_raster_draws* draws, const float* depth, const ur_gbuffer_targets* targets,
                              uint32_t w, uint32_t h, uint32_t row0, uint32_t rows, uint32_t flags, uint32_t key_triangle_bits, uint32_t* stats6,
                              const ur_material* materials, uint32_t material_count)
{
    return gbuffer_entry("ur_gbuffer_pass_materials", "ur_gbuffer_pass_materials_parts", ctx, view, projection, draws, depth, targets, w, h, row0, rows, flags,
                         key_triangle_bits, stats6, UR_GBUFFER_PART_RASTER | UR_GBUFFER_PART_RESOLVE, materials, material_count);
}

int ur_gbuffer_pass_parts(ur_ctx* ctx, const float* view, const float* projection, const ur_raster_draws* draws, const float* depth, const ur_gbuffer_targets* targets,
                          uint32_t w, uint32_t h, uint32_t row0, uint32_t rows, uint32_t flags, uint32_t key_triangle_bits, uint32_t* stats6, uint32_t parts)
{
    return gbuffer_entry("ur_gbuffer_pass", "ur_gbuffer_pass_parts", ctx, view, projection, draws, depth, targets, w, h, row0, rows, flags, key_triangle_bits, stats6, parts,
                         nullptr, 0u);
}

int ur_gbuffer_pass(ur_ctx* ctx, const float* view, const float* projection, const ur_raster_draws* draws, const float* depth, const ur_gbuffer_targets* targets,
                    uint32_t w, uint32_t h, uint32_t row0, uint32_t rows, uint32_t flags, uint32_t key_triangle_bits, uint32_t* stats6)
{
    return gbuffer_entry("ur_gbuffer_pass", "ur_gbuffer_pass_parts", ctx, view, projection, draws, depth, targets, w, h, row0, rows, flags, key_triangle_bits, stats6,
                         UR_GBUFFER_PART_RASTER | UR_GBUFFER_PART_RESOLVE, nullptr, 0u);
}

} // extern "C"
