// What every consumer of a visibility key does alike, operation for operation (DESIGN.md sections 3.9 to 3.12): GBuffer's resolve
// (csrc/gbuffer_resolve.hip), the Forward pass' resolve (csrc/forward_resolve.hip) and the alpha test of the masked raster (csrc/raster_mask.hip).
// The key's way back to its draw, the fill of the sampler's tables, the quad's differences, and the two resolves' loop over the four maps,
// tangent frame and material factors; from the triangle to the texel's weights it is gbuffer_interp.h, the sampler texture_sample.h.
// Device inline functions only. The two resolves' vertex stage is not here: DESIGN.md section 3.14 says why.
#pragma once

#include "gbuffer_interp.h"
#include "texture_sample.h"

namespace ur_raster {

// The key's halves: the slot of its command (returned) and the triangle `t` within the draw. The ordinal is the slot, or under a visible
// list the position in the list. MASKED: texel i's key is a position in the masked selection's list iff its 64-bit word
// is not 0. P: the resolves' ur::KeyParams (csrc/gbuffer_resolve.h) or the raster's MaskedParams
template <bool MASKED, class P>
__device__ __forceinline__ uint32_t key_slot(const P& p, uint32_t key, uint32_t i, uint32_t& t)
{
    const uint32_t ordinal = (key >> p.key_bits) - 1u;
    t = key & ((1u << p.key_bits) - 1u);
    uint32_t slot = p.mode == 1u ? p.visible_idx[ordinal] - p.index_base : ordinal;
    if constexpr (MASKED) {
        if (p.keys64[i] != 0ull) slot = p.mask_mode == 1u ? p.mask_visible_idx[ordinal] - p.mask_index_base : ordinal;
    }
    return slot;
}

// What the command in `slot` says of triangle t: the vertex buffer and its stride, the index buffer and the triangle's first index, the
// draw's constants (ur_scene_constants as floats) and their World matrix
struct KeyDraw {
    const uint8_t* vertices;
    const uint32_t* indices;
    const float* cb;
    float W[16];
    uint32_t stride;
    uint64_t first;
    long long base_vertex;
};

__device__ __forceinline__ KeyDraw key_draw(const uint8_t* commands, uint32_t slot, uint32_t t)
{
    const u32x4_t* cmd = reinterpret_cast<const u32x4_t*>(commands + (size_t)slot * UR_INDIRECT_COMMAND_STRIDE);
    const u32x4_t c0 = cmd[0], c1 = cmd[1], c2 = cmd[2], c3 = cmd[3];
    KeyDraw d;
    d.vertices = reinterpret_cast<const uint8_t*>((uint64_t)c0.x | ((uint64_t)c0.y << 32));
    d.indices = reinterpret_cast<const uint32_t*>((uint64_t)c1.x | ((uint64_t)c1.y << 32));
    d.cb = reinterpret_cast<const float*>((uint64_t)c2.x | ((uint64_t)c2.y << 32));
    d.stride = c0.w;
    d.first = (uint64_t)c3.x + 3ull * t;
    d.base_vertex = (int)c3.y;
#pragma unroll
    for (int k = 0; k < 16; ++k) d.W[k] = d.cb[k];
    return d;
}

// The sampler's tables (texture_sample.h) into LDS, by a block of kThreads = 256: code / 255, the level thresholds and, with DECODE, the
// sRGB decode. The alpha test samples channel A alone, which never goes through the decode: without DECODE `decode` is not read
template <bool DECODE>
__device__ __forceinline__ void fill_sampler_tables(float* lds, const float* decode, const float* lod)
{
    if constexpr (DECODE) lds[kLdsDecode + threadIdx.x] = decode[threadIdx.x];
    lds[kLdsUnorm + threadIdx.x] = (float)threadIdx.x / 255.0f;
    if (threadIdx.x < 128u) lds[kLdsLod + threadIdx.x] = lod[min(threadIdx.x, 126u)];
}

// The quad's differences of a transformed coordinate from its values at the centre (point 0), the horizontal (1) and the vertical (2)
// partner: value(odd) - value(even)
__device__ __forceinline__ void quad_differences(const float (&tu)[3], const float (&tv)[3], bool odd_column, bool odd_row, float& dxu, float& dxv, float& dyu, float& dyv)
{
    dxu = odd_column ? tu[0] - tu[1] : tu[1] - tu[0];
    dxv = odd_column ? tv[0] - tv[1] : tv[1] - tv[0];
    dyu = odd_row ? tu[0] - tu[2] : tu[2] - tu[0];
    dyv = odd_row ? tv[0] - tv[2] : tv[2] - tv[0];
}

// The samples of the maps t0 base colour, t1 metallic-roughness, t2 normal, t3 emissive whose bit is set in `bits`, at quad_texcoords'
// (pu, pv); a map without a valid descriptor loses its bit and keeps the caller's value. The two shaders differ in SPLIT (sample_map) and
// MR_AT_BASE: ForwardPS.hlsl:103 samples the metallic-roughness map at the base colour's transform. The results are written by select: a
// conditional store through a reference becomes a store to a selected address and keeps the caller's arrays in scratch
template <bool SPLIT, bool MR_AT_BASE>
__device__ __forceinline__ void sample_maps(const ur_material* material, uint32_t& bits, const float* cb, const float (&pu)[3], const float (&pv)[3], bool odd_column, bool odd_row,
                                            const float* lds, float (&base)[3], float (&mr)[3], float (&nm)[3], float (&em)[3])
{
#pragma unroll 1
    for (uint32_t map = 0u; map < 4u; ++map) {
        const uint32_t bit = map == 0u ? UR_MATERIAL_BASE_COLOR_MAP : (map == 1u ? UR_MATERIAL_METALLIC_ROUGHNESS_MAP : (map == 2u ? UR_MATERIAL_NORMAL_MAP : UR_MATERIAL_EMISSIVE_MAP));
        if (__ballot((bits & bit) != 0u) == 0ull) continue;
        if ((bits & bit) == 0u) continue;
        const u32x4_t desc = reinterpret_cast<const u32x4_t*>(material)[map];
        if (!valid_texture(desc)) { bits &= ~bit; continue; }
        const uint32_t at = MR_AT_BASE && map == 1u ? 112u : 112u + 8u * map; // the map's OffsetScale and Rotation in ur_scene_constants
        float tu[3], tv[3];
#pragma unroll
        for (int point = 0; point < 3; ++point) texture_transform(cb, at, pu[point], pv[point], tu[point], tv[point]);
        float dxu, dxv, dyu, dyv, s[3];
        quad_differences(tu, tv, odd_column, odd_row, dxu, dxv, dyu, dyv);
        sample_map<0, 3, SPLIT>(desc, tu[0], tv[0], dxu, dxv, dyu, dyv, lds, s);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            base[k] = map == 0u ? s[k] : base[k];
            mr[k] = map == 1u ? s[k] : mr[k];
            nm[k] = map == 2u ? s[k] : nm[k];
            em[k] = map == 3u ? s[k] : em[k];
        }
    }
}

// ComputeWorldNormal's frame around the unit normal vn: the vertices' tangents tg under the weights b, Gram-Schmidt against vn (t), and
// cross(vn, t) normalised times the handedness (bt)
__device__ __forceinline__ void tangent_frame(const float (&vn)[3], const float (&b)[3], const float (&tg)[3][4], float (&t)[3], float (&bt)[3])
{
    float tan4[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) tan4[k] = (b[0] * tg[0][k] + b[1] * tg[1][k]) + b[2] * tg[2][k];
    const float dt = (vn[0] * tan4[0] + vn[1] * tan4[1]) + vn[2] * tan4[2];
    const float u0 = tan4[0] - vn[0] * dt, u1 = tan4[1] - vn[1] * dt, u2 = tan4[2] - vn[2] * dt;
    const float ul = sqrtf((u0 * u0 + u1 * u1) + u2 * u2);
    t[0] = u0 / ul; t[1] = u1 / ul; t[2] = u2 / ul;
    const float c0 = vn[1] * t[2] - vn[2] * t[1], c1 = vn[2] * t[0] - vn[0] * t[2], c2 = vn[0] * t[1] - vn[1] * t[0];
    const float cl = sqrtf((c0 * c0 + c1 * c1) + c2 * c2);
    bt[0] = (c0 / cl) * tan4[3]; bt[1] = (c1 / cl) * tan4[3]; bt[2] = (c2 / cl) * tan4[3];
}

// ... and the tangent-space vector e, which each shader forms its own way, taken through the frame and normalised
__device__ __forceinline__ void tangent_to_world(const float (&e)[3], const float (&t)[3], const float (&bt)[3], const float (&vn)[3], float (&out)[3])
{
    const float w0 = (e[0] * t[0] + e[1] * bt[0]) + e[2] * vn[0], w1 = (e[0] * t[1] + e[1] * bt[1]) + e[2] * vn[1], w2 = (e[0] * t[2] + e[1] * bt[2]) + e[2] * vn[2];
    const float wl = sqrtf((w0 * w0 + w1 * w1) + w2 * w2);
    out[0] = w0 / wl; out[1] = w1 / wl; out[2] = w2 / wl;
}

// The material's factors times its maps' samples, for the maps whose bit is left in `bits`: G is roughness, B metallic
__device__ __forceinline__ void apply_map_factors(uint32_t bits, const float (&base)[3], const float (&mr)[3], const float (&em)[3], float (&albedo)[3], float& metallic,
                                                  float& roughness, float (&emissive)[3])
{
    if (bits & UR_MATERIAL_BASE_COLOR_MAP) { albedo[0] = albedo[0] * base[0]; albedo[1] = albedo[1] * base[1]; albedo[2] = albedo[2] * base[2]; }
    if (bits & UR_MATERIAL_METALLIC_ROUGHNESS_MAP) { metallic = metallic * mr[2]; roughness = roughness * mr[1]; }
    if (bits & UR_MATERIAL_EMISSIVE_MAP) { emissive[0] = emissive[0] * em[0]; emissive[1] = emissive[1] * em[1]; emissive[2] = emissive[2] * em[2]; }
}

} // namespace ur_raster
