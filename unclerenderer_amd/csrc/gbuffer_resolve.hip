// GBuffer's resolve for gfx950 — a lane per texel of the band turns the winning visibility key (csrc/raster.hip) into the render
// targets: it fetches the key's triangle again (csrc/visibility_key.h), restates the near clip with a weight row per polygon vertex,
// interpolates the attributes perspective-correct and runs the base pass' pixel shader (Shaders/DeferredBasePass.hlsl), with or without
// ObjectId and texture maps (csrc/texture_sample.h). DESIGN.md sections 3.9 and 3.10 are its rule, tests/gbuffer_ref.py the restatement.
// Built with -ffp-contract=off. The entry points that fill its arguments are csrc/gbuffer_api.hip's.

#include "gbuffer_resolve.h"
#include "resolve_pack.h"
#include "ur_device.h"
#include "visibility_key.h"

namespace {

using namespace ur_raster;
using ur::ResolveParams;

static_assert(sizeof(ur_texture2d) == 16 && sizeof(ur_material) == 80, "ur_material is 80 bytes");

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

template <bool OBJECT_ID, bool MAPS, bool MASKED>
__global__ __launch_bounds__(kThreads) void gbuffer_resolve_kernel(ResolveParams p)
{
    __shared__ float table[256];
    __shared__ float sampler_tables[MAPS ? kLdsFloats : 1u];
    table[threadIdx.x] = p.table[min(threadIdx.x, 254u)];
    if constexpr (MAPS) fill_sampler_tables<true>(sampler_tables, p.decode, p.lod);
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
    uint32_t t;
    const uint32_t slot = key_slot<MASKED>(p, key, i, t);
    const KeyDraw d = key_draw(p.commands, slot, t);
    const float* cb = d.cb;
    const float (&W)[16] = d.W;

    // ---- the three vertices: rule 1 (world and clip position), the world normal, the colour. (One text with the Forward resolve's vertex
    // stage, csrc/forward_resolve.hip, and not one function: shared, it costs that kernel scratch. DESIGN.md 3.14 has the table)
    float c[3][4], wp[3][3], wn[3][3], col[3][3];
    [[maybe_unused]] float uv[3][2], tg[3][4]; // MAPS: TEXCOORD and the vertex shader's tangent
#pragma unroll
    for (int v = 0; v < 3; ++v) {
        const uint64_t vi = (uint64_t)(d.base_vertex + (long long)d.indices[d.first + (uint32_t)v]);
        const f32x4u_t* vp = reinterpret_cast<const f32x4u_t*>(d.vertices + vi * d.stride);
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

    // ---- the material of the slot, its valid maps, and the samples
    [[maybe_unused]] uint32_t bits = 0u;
    [[maybe_unused]] float base[3] = {1.0f, 1.0f, 1.0f}, mr[3] = {1.0f, 1.0f, 1.0f}, nm[3] = {0.5f, 0.5f, 1.0f}, em[3] = {1.0f, 1.0f, 1.0f};
    if constexpr (MAPS) {
        if (slot < p.material_count) bits = reinterpret_cast<const uint32_t*>(p.materials + slot)[16] & 15u;
        if (__ballot(bits != 0u) != 0ull) {
            const bool odd_column = (column & 1u) != 0u, odd_row = ((p.row0 + row) & 1u) != 0u;
            float pu[3], pv[3]; // TEXCOORD at the centre, the horizontal and the vertical partner
            quad_texcoords(pc, B, uv, odd_column, odd_row, pu, pv);
            sample_maps<true, false>(p.materials + slot, bits, cb, pu, pv, odd_column, odd_row, sampler_tables, base, mr, nm, em);
        }
    }

    // ---- the pixel shader (DeferredBasePass.hlsl:80-149)
    const float nl = sqrtf((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
    const float vn[3] = {n[0] / nl, n[1] / nl, n[2] / nl};
    float wnrm[3] = {vn[0], vn[1], vn[2]};
    float albedo[3] = {cb[64] * colour[0], cb[65] * colour[1], cb[66] * colour[2]};
    float metallic = cb[104], roughness = cb[105];
    float emissive[3] = {cb[80], cb[81], cb[82]};
    if constexpr (MAPS) {
        if (bits & UR_MATERIAL_NORMAL_MAP) {
            float tn[3], bt[3];
            tangent_frame(vn, b, tg, tn, bt);
            // the tangent-space vector: the map's red and green, and the blue they leave to a unit vector (the Forward shader takes the map's)
            const float nr = nm[0] * 2.0f - 1.0f, ng = nm[1] * 2.0f - 1.0f;
            const float one_minus = 1.0f - (nr * nr + ng * ng);
            const float nz = sqrtf(one_minus > 0.0f ? fminf(one_minus, 1.0f) : 0.0f); // saturate
            const bool flat = sqrtf((nr * nr + ng * ng) + nz * nz) < 1e-5f;
            const float e[3] = {flat ? 0.0f : nr, flat ? 0.0f : ng, flat ? 1.0f : nz};
            tangent_to_world(e, tn, bt, vn, wnrm);
        }
        apply_map_factors(bits, base, mr, em, albedo, metallic, roughness, emissive);
    }
    float m[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) m[k] = (wnrm[0] * p.V[k] + wnrm[1] * p.V[4 + k]) + wnrm[2] * p.V[8 + k];
    const float ml = sqrtf((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
    const float view_depth = -(((wpos[0] * p.V[2] + wpos[1] * p.V[6]) + wpos[2] * p.V[10]) + p.V[14]);
    const uint32_t r8 = srgb_code(table, albedo[0]), g8 = srgb_code(table, albedo[1]), b8 = srgb_code(table, albedo[2]);
    ur::store_once_b64(p.gbuf_a + i, pack_half4(m[0] / ml, m[1] / ml, m[2] / ml, view_depth));
    ur::store_once_b64(p.gbuf_b + i, pack_half4(0.04f, metallic, roughness, 1.0f));
    ur::store_once_b32(p.gbuf_c + i, r8 | (g8 << 8) | (b8 << 16) | 0xFF000000u);
    ur::store_once_b64(p.hdr + i, pack_half4(emissive[0], emissive[1], emissive[2], 1.0f));
    if constexpr (OBJECT_ID) ur::store_once_b32(p.object_id + i, reinterpret_cast<const uint32_t*>(cb)[148]);
}

// The ObjectId pass' resolve, a lane per texel of the band: key -> ordinal -> slot -> command -> dword 148 of its
// constants, 0 for key 0. No vertex is loaded and no LDS used
__global__ __launch_bounds__(kThreads) void object_id_resolve_kernel(ur::ObjectIdParams p)
{
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= p.n) return;
    const uint32_t key = p.keys[i];
    uint32_t id = 0u;
    if (key != 0u) {
        uint32_t t;
        const uint32_t slot = key_slot<false>(p, key, i, t);
        const u32x4_t c2 = reinterpret_cast<const u32x4_t*>(p.commands + (size_t)slot * UR_INDIRECT_COMMAND_STRIDE)[2];
        id = reinterpret_cast<const uint32_t*>((uint64_t)c2.x | ((uint64_t)c2.y << 32))[148];
    }
    ur::store_once_b32(p.object_id + i, id);
}

template <bool OBJECT_ID, bool MAPS, bool MASKED>
void launch(ur_ctx* ctx, const ResolveParams& p)
{
    hipLaunchKernelGGL((gbuffer_resolve_kernel<OBJECT_ID, MAPS, MASKED>), dim3((p.n + kThreads - 1u) / kThreads), dim3(kThreads), 0, ctx->stream, p);
}

} // namespace

int ur::launch_gbuffer_resolve(ur_ctx* ctx, const ResolveParams& p, bool object_id, bool maps, bool masked)
{
    if (masked && maps) launch<false, true, true>(ctx, p);
    else if (masked) launch<false, false, true>(ctx, p);
    else if (object_id && maps) launch<true, true, false>(ctx, p);
    else if (object_id) launch<true, false, false>(ctx, p);
    else if (maps) launch<false, true, false>(ctx, p);
    else launch<false, false, false>(ctx, p);
    UR_HIP_TRY(hipGetLastError());
    return UR_OK;
}

int ur::launch_object_id_resolve(ur_ctx* ctx, const ObjectIdParams& p)
{
    hipLaunchKernelGGL(object_id_resolve_kernel, dim3((p.n + kThreads - 1u) / kThreads), dim3(kThreads), 0, ctx->stream, p);
    UR_HIP_TRY(hipGetLastError());
    return UR_OK;
}
