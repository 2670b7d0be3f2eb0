// GBuffer's alpha-masked draws for gfx950 (restated in tests/gbuffer_mask_ref.py): a third keyed policy of the
// raster kernels (csrc/raster_kernels.h). A fragment that passes the depth test competes for a 64-bit word per texel,
// (depth bits << 32) | key, and runs the base pass' alpha test (alpha_discards below, with the resolves' front end: visibility_key.h,
// gbuffer_interp.h, texture_sample.h) only when its word is above the texel's; a merge launch then folds the words into the opaque
// draws' key image and raises the depth where a masked fragment won. Built with -ffp-contract=off.

#include "raster_kernels.h"

namespace {

// Rule 3 of section 3.11 for the fragment of the triangle `key` names at the texel (px, py): the triangle is fetched again from the key as
// the resolve fetches it, COLOR.a and TEXCOORD interpolated with the resolve's weights, channel A of the base-colour map sampled with the
// resolve's sampler. True iff alpha < AlphaCutoff (false for a NaN on either side).
template <class P>
__device__ __forceinline__ bool alpha_discards(const AlphaCtx& a, uint32_t key, int px, int py)
{
    const MaskedParams& p = *a.p;
    uint32_t t;
    const uint32_t slot = key_slot<false>(p, key, 0u, t); // (the masked draws' own selection: no detour)
    uint32_t bits = 0u;
    if (p.mask.materials != nullptr && slot < p.mask.material_count) bits = reinterpret_cast<const uint32_t*>(p.mask.materials + slot)[16];
    if ((bits & UR_MATERIAL_ALPHA_MASK) == 0u) return false;
    const KeyDraw d = key_draw(p.commands, slot, t);
    const float* cb = d.cb;
    const float (&W)[16] = d.W;
    float c[3][4], uv[3][2], va[3]; // clip position, TEXCOORD, COLOR.a
#pragma unroll
    for (int v = 0; v < 3; ++v) {
        const uint64_t vi = (uint64_t)(d.base_vertex + (long long)d.indices[d.first + (uint32_t)v]);
        const float* vp = reinterpret_cast<const float*>(d.vertices + vi * d.stride);
        P::project(vp, W, p, c[v]);
        uv[v][0] = vp[6]; uv[v][1] = vp[7];
        va[v] = vp[15];
    }
    float SX[4], SY[4], vw[4], B[4][3];
    bool one;
    clip_polygon(c, p.half_w, p.half_h, SX, SY, vw, B, one);
    Piece pc;
    covering_piece(SX, SY, vw, one, 256 * px + 128, 256 * py + 128, pc);
    float b[3];
    piece_weights(pc, pc.l0, pc.l1, pc.l2, B, b);
    float alpha = cb[106] * ((b[0] * va[0] + b[1] * va[1]) + b[2] * va[2]); // BaseColorAlpha * COLOR.a
    if (bits & UR_MATERIAL_BASE_COLOR_MAP) {
        const u32x4_t desc = reinterpret_cast<const u32x4_t*>(p.mask.materials + slot)[0];
        if (valid_texture(desc)) {
            const bool odd_column = ((uint32_t)px & 1u) != 0u, odd_row = ((uint32_t)py & 1u) != 0u;
            float pu[3], pv[3], tu[3], tv[3];
            quad_texcoords(pc, B, uv, odd_column, odd_row, pu, pv);
#pragma unroll
            for (int point = 0; point < 3; ++point) texture_transform(cb, 112u, pu[point], pv[point], tu[point], tv[point]);
            float dxu, dxv, dyu, dyv, sa[1];
            quad_differences(tu, tv, odd_column, odd_row, dxu, dxv, dyu, dyv);
            sample_map<3, 1>(desc, tu[0], tv[0], dxu, dxv, dyu, dyv, a.lds, sa);
            alpha = alpha * sa[0];
        }
    }
    return alpha < cb[107]; // AlphaCutoff
}

// The large-triangle kernel of the masked policy: what the alpha test reads rides in the parameters, its tables in LDS
template <class P>
__global__ __launch_bounds__(kThreads) void large_masked_kernel(MaskedParams p)
{
    __shared__ float sampler_tables[kLdsFloats];
    fill_sampler_tables<false>(sampler_tables, nullptr, p.mask.lod);
    __syncthreads();
    large_body<P>(p.queue, p.queue_cap, p.map, p.w, p.depth, p.row0, AlphaCtx{&p, sampler_tables});
}

// Rule 5 of section 3.11, a lane per texel of the band: the masked word against the opaque key and the depth; where the masked fragment
// wins, the key image takes its key and the depth its depth, where it loses its word is set to 0 (a word that is left says which selection
// the texel's key belongs to). `depth` points at the band's first row. `won` is added to once per wave.
__global__ __launch_bounds__(kThreads) void mask_merge_kernel(unsigned long long* __restrict__ keys64, uint32_t* __restrict__ keys, uint32_t* __restrict__ depth,
                                                              uint32_t n, uint32_t* __restrict__ won)
{
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    bool wins = false;
    if (i < n) {
        const unsigned long long km = keys64[i];
        const uint32_t hi = (uint32_t)(km >> 32), lo = (uint32_t)km;
        wins = km != 0ull && (hi > depth[i] || lo > keys[i]);
        if (wins) { keys[i] = lo; depth[i] = hi; }
        else if (km != 0ull) keys64[i] = 0ull;
    }
    const uint32_t count = (uint32_t)__popcll(__ballot(wins));
    if (won != nullptr && count != 0u && (threadIdx.x & 63u) == 0u) (void)__hip_atomic_fetch_add(won, count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

} // namespace

int ur::launch_masked_raster(ur_ctx* ctx, const float* view, const float* projection, const ur_raster_draws* draws, float* depth, uint64_t* keys64, uint32_t* keys,
                             uint32_t w, uint32_t h, uint32_t row0, uint32_t rows, uint32_t key_bits, bool d24, uint32_t* stats, const ur_material* materials,
                             uint32_t material_count, uint32_t* won)
{
    const VisArgs vis{depth, row0, rows, key_bits};
    const MaskArgs mask{materials, material_count, ctx->lod_table};
    uint32_t* words = reinterpret_cast<uint32_t*>(keys64);
    const uint32_t n = w * rows;
    const int rc = d24 ? launch_raster<MaskPolicy<true>>(ctx, view, projection, draws, words, 2u * n, w, h, 0.0f, stats, &vis, &mask)
                       : launch_raster<MaskPolicy<false>>(ctx, view, projection, draws, words, 2u * n, w, h, 0.0f, stats, &vis, &mask);
    if (rc != UR_OK) return rc;
    hipLaunchKernelGGL(mask_merge_kernel, dim3((n + kThreads - 1u) / kThreads), dim3(kThreads), 0, ctx->stream, reinterpret_cast<unsigned long long*>(keys64), keys,
                       reinterpret_cast<uint32_t*>(depth) + (size_t)row0 * w, n, won);
    UR_HIP_TRY(hipGetLastError());
    return UR_OK;
}
