// The static sampler of the textured GBuffer resolve (DESIGN.md section 3.10 is its rule, tests/gbuffer_tex_ref.py the restatement):
// ApplyTextureTransform, wrap addressing, one bilinear sample, and the footprint / level of detail / trilinear probes of one map, as
// device inline functions over tables the including kernel has put into LDS (layout below). A texel is an RGBA8 code word: read as it
// lies, or decoded from its BC1 / BC3 / BC5 block by csrc/bc_decode.h. csrc/gbuffer_resolve.hip samples R, G and B
// with it, the masked raster's alpha test (csrc/raster_mask.hip) channel A: the same sampler with another output.
#pragma once

#include "bc_decode.h"
#include "raster_rule.h"

#include "../../include/ur_raster.h"

namespace {

using ur_raster::u32x4_t;

static_assert(ur_bc::kBC1 == UR_TEXTURE_BC1_UNORM && ur_bc::kBC1Srgb == UR_TEXTURE_BC1_UNORM_SRGB && ur_bc::kBC3 == UR_TEXTURE_BC3_UNORM &&
              ur_bc::kBC3Srgb == UR_TEXTURE_BC3_UNORM_SRGB && ur_bc::kBC5 == UR_TEXTURE_BC5_UNORM, "csrc/bc_decode.h names the header's format codes");

constexpr uint32_t kLdsDecode = 0u, kLdsUnorm = 256u, kLdsLod = 512u, kLdsFloats = 640u; // the sampler's tables in LDS, in floats

// (i + 0.5) / N - 0.5 for N = 1, 2, 3, 4, i ascending
__constant__ float kProbeOffset[10] = {0.0f, -0.25f, 0.25f, -0.33333334f, 0.0f, 0.33333334f, -0.375f, -0.125f, 0.125f, 0.375f};

// ApplyTextureTransform with the constant vectors at cb[at .. at + 8)
__device__ __forceinline__ void texture_transform(const float* __restrict__ cb, uint32_t at, float u, float v, float& tu, float& tv)
{
    const float su = u * cb[at + 2u], sv = v * cb[at + 3u];
    const float ru = su * cb[at + 4u] - sv * cb[at + 5u], rv = su * cb[at + 5u] + sv * cb[at + 4u];
    tu = ru + cb[at + 0u];
    tv = rv + cb[at + 1u];
}

// x = u * size - 0.5 -> the two wrapped texel indices and the weight; a coordinate that is not finite, or beyond 2^30 texels, counts as 0
__device__ __forceinline__ void wrap_pair(float u, uint32_t size, uint32_t& i0, uint32_t& i1, float& f)
{
    float x = u * (float)size - 0.5f;
    if (!(fabsf(x) <= 1073741824.0f)) x = 0.0f;
    const float x0 = floorf(x);
    f = x - x0;
    int r = (int)x0 % (int)size;
    if (r < 0) r += (int)size;
    i0 = (uint32_t)r;
    i1 = i0 + 1u == size ? 0u : i0 + 1u;
}

// The four taps of a BC level as RGBA8 code words (csrc/bc_decode.h is the decode): per tap one 8-byte load of the half of
// its block that the channels [C0, C0 + N) need - BC1's block, BC3's colour half for R, G, B and its alpha half for A, BC5's red half -;
// the other half is loaded only where both are needed (BC5's green, BC3 with colour and alpha). BC5's alpha alone loads nothing.
// `format` is the lane's own: neighbouring lanes may hold different ones. The taps go a texel row at a time through a loop that stays
// rolled, two loads in flight, then two decodes: four at once keep eight more registers live over the loads and double the decode's
// temporaries, and the forward resolve has none to spare at three waves per SIMD (DESIGN.md 3.13 has the figures).
template <int C0, int N>
__device__ __forceinline__ void bc_taps(const uint8_t* __restrict__ level, uint32_t wd, uint32_t format, uint32_t x0, uint32_t x1, uint32_t y0, uint32_t y1, uint32_t (&t)[4])
{
    constexpr bool kColour = C0 < 3, kAlpha = C0 + N > 3;
    const bool bc1 = ur_bc::is_bc1(format), bc5 = format == ur_bc::kBC5;
    if (!kColour && bc5) { t[0] = t[1] = t[2] = t[3] = 0xFF000000u; return; }
    const uint32_t across = ur_bc::blocks_across(wd), shift = bc1 ? 3u : 4u;
    const uint32_t first = kColour && !bc1 && !bc5 ? 8u : 0u; // BC3's colour block is its second half
#pragma unroll 1
    for (int row = 0; row < 2; ++row) {
        const uint32_t y = row == 0 ? y0 : y1;
        const uint8_t* a = level + (ur_bc::block_of(x0, y, across) << shift);
        const uint8_t* b = level + (ur_bc::block_of(x1, y, across) << shift);
        const uint32_t na = ur_bc::index_in_block(x0, y), nb = ur_bc::index_in_block(x1, y);
        const uint64_t ha = *reinterpret_cast<const uint64_t*>(a + first), hb = *reinterpret_cast<const uint64_t*>(b + first);
        uint32_t ta, tb;
        if (bc5) { // (colour is asked for: R from bytes 0-7, G from bytes 8-15)
            ta = ur_bc::alpha_code(ha, na) | 0xFF000000u;
            tb = ur_bc::alpha_code(hb, nb) | 0xFF000000u;
            if (C0 + N > 1) {
                const uint64_t ga = *reinterpret_cast<const uint64_t*>(a + 8), gb = *reinterpret_cast<const uint64_t*>(b + 8);
                ta |= ur_bc::alpha_code(ga, na) << 8;
                tb |= ur_bc::alpha_code(gb, nb) << 8;
            }
        } else if (kColour) {
            ta = ur_bc::colour_word(ha, na, !bc1);
            tb = ur_bc::colour_word(hb, nb, !bc1);
            if (kAlpha && !bc1) { // BC3's alpha beside its colour: the other half
                const uint64_t aa = *reinterpret_cast<const uint64_t*>(a), ab = *reinterpret_cast<const uint64_t*>(b);
                ta = (ta & 0x00FFFFFFu) | (ur_bc::alpha_code(aa, na) << 24);
                tb = (tb & 0x00FFFFFFu) | (ur_bc::alpha_code(ab, nb) << 24);
            }
        } else {
            ta = bc1 ? ur_bc::colour_word(ha, na, false) : ur_bc::alpha_code(ha, na) << 24;
            tb = bc1 ? ur_bc::colour_word(hb, nb, false) : ur_bc::alpha_code(hb, nb) << 24;
        }
        if (row == 0) { t[0] = ta; t[1] = tb; } else { t[2] = ta; t[3] = tb; }
    }
}

// One bilinear sample of a level: the channels [C0, C0 + N) decoded through `tab` (LDS: the sRGB decode or code / 255). A tap is an RGBA8
// code word whatever the format: read as it lies (RGBA8), or decoded from its block (bc_taps). BC = false: no lane holds a BC format
template <int C0, int N, bool BC>
__device__ __forceinline__ void bilinear(const uint8_t* __restrict__ level, uint32_t wd, uint32_t hd, uint32_t format, float u, float v, const float* tab, float (&out)[N])
{
    uint32_t x0, x1, y0, y1;
    float fx, fy;
    wrap_pair(u, wd, x0, x1, fx);
    wrap_pair(v, hd, y0, y1, fy);
    uint32_t t[4];
    if (BC && ur_bc::is_bc(format)) bc_taps<C0, N>(level, wd, format, x0, x1, y0, y1, t);
    else {
        const uint32_t* r0 = reinterpret_cast<const uint32_t*>(level) + (size_t)y0 * wd;
        const uint32_t* r1 = reinterpret_cast<const uint32_t*>(level) + (size_t)y1 * wd;
        t[0] = r0[x0]; t[1] = r0[x1]; t[2] = r1[x0]; t[3] = r1[x1];
    }
#pragma unroll
    for (int c = 0; c < N; ++c) {
        const float a = tab[(t[0] >> (8 * (C0 + c))) & 255u], b = tab[(t[1] >> (8 * (C0 + c))) & 255u];
        const float d = tab[(t[2] >> (8 * (C0 + c))) & 255u], e = tab[(t[3] >> (8 * (C0 + c))) & 255u];
        const float top = a + fx * (b - a), bottom = d + fx * (e - d);
        out[c] = top + fy * (bottom - top);
    }
}

// What sample_map found for a map: the level d and the fraction towards d + 1, the probe count and the major axis' differences
struct Lod { uint32_t d; float f; uint32_t n; float mu, mv; };

// The probes of one map: the two levels' addresses and the trilinear samples along the major axis. BC = false: every lane's format is RGBA8
template <int C0, int N, bool BC>
__device__ __forceinline__ void gather_levels(const uint8_t* texels, uint32_t width, uint32_t height, uint32_t mips, uint32_t format, const Lod lod, float u, float v,
                                              const float* lds, float (&out)[N])
{
    const uint32_t d = lod.d, n = lod.n;
    const float f = lod.f, mu = lod.mu, mv = lod.mv;
    // a dimension is at most 65535, so every level from 16 on is 1 x 1: the shift count stays below the word's width for any `mips`.
    // A level is counted in units of 4 bytes (RGBA8: its texels), 8 or 16 bytes (BC: its 4 x 4 blocks, ur_bc::level_blocks)
    const bool bc = BC && ur_bc::is_bc(format);
    const uint32_t unit = bc ? ur_bc::block_bytes(format) : 4u;
    size_t offset = 0u;
    for (uint32_t k = 0u; k < d; ++k) {
        const uint32_t wk = ur_bc::level_size(width, k), hk = ur_bc::level_size(height, k);
        offset += bc ? (size_t)ur_bc::blocks_across(wk) * ur_bc::blocks_across(hk) : (size_t)wk * hk;
    }
    const uint32_t wd = ur_bc::level_size(width, d), hd = ur_bc::level_size(height, d);
    const uint32_t d1 = min(d + 1u, mips - 1u);
    const uint32_t we = ur_bc::level_size(width, d1), he = ur_bc::level_size(height, d1);
    const uint8_t* level0 = texels + offset * unit;
    const uint8_t* level1 = d1 == d ? level0 : level0 + (bc ? (size_t)ur_bc::blocks_across(wd) * ur_bc::blocks_across(hd) : (size_t)wd * hd) * unit;
    const float* tab = lds + (C0 != 3 && ur_bc::is_srgb(format) ? kLdsDecode : kLdsUnorm);
    float sum[N] = {};
    for (uint32_t i = 0u; i < n; ++i) {
        const float o = kProbeOffset[n * (n - 1u) / 2u + i];
        const float pu = u + mu * o, pv = v + mv * o;
        float s[N];
        bilinear<C0, N, BC>(level0, wd, hd, format, pu, pv, tab, s);
        if (f != 0.0f) { // (lo + 0 * (hi - lo) is lo: every value here is finite and no zero is negative)
            float t[N];
            bilinear<C0, N, BC>(level1, we, he, format, pu, pv, tab, t);
#pragma unroll
            for (int c = 0; c < N; ++c) s[c] = s[c] + f * (t[c] - s[c]);
        }
#pragma unroll
        for (int c = 0; c < N; ++c) sum[c] = i == 0u ? s[c] : sum[c] + s[c];
    }
    const float fn = (float)n;
#pragma unroll
    for (int c = 0; c < N; ++c) out[c] = sum[c] / fn;
}

// The static sampler on one map: footprint, level of detail, up to four trilinear probes. (u, v) the centre's coordinate, (dxu, dxv) and
// (dyu, dyv) the quad's differences; `desc` a valid descriptor's four dwords; `lds` the tables. The output is the channels [C0, C0 + N):
// R, G, B for a map of the resolve, A alone (C0 = 3: code / 255 whatever the format, and the decode table is not read) for the alpha test.
// SPLIT: see the end of the function
template <int C0 = 0, int N = 3, bool SPLIT = true>
__device__ __forceinline__ void sample_map(const u32x4_t desc, float u, float v, float dxu, float dxv, float dyu, float dyv, const float* lds, float (&out)[N])
{
    const uint8_t* texels = reinterpret_cast<const uint8_t*>((uint64_t)desc.x | ((uint64_t)desc.y << 32));
    const uint32_t width = desc.z & 0xFFFFu, height = desc.z >> 16, mips = desc.w & 0xFFu, format = (desc.w >> 8) & 0xFFu;
    const float fw = (float)width, fh = (float)height;
    const float axu = dxu * fw, axv = dxv * fh, ayu = dyu * fw, ayv = dyv * fh;
    const float px2 = axu * axu + axv * axv, py2 = ayu * ayu + ayv * ayv;
    const bool ymajor = py2 > px2; // a tie goes to x
    const float pmax2 = ymajor ? py2 : px2, pmin2 = ymajor ? px2 : py2;
    const uint32_t n = pmax2 <= pmin2 ? 1u : (pmax2 <= 4.0f * pmin2 ? 2u : (pmax2 <= 9.0f * pmin2 ? 3u : 4u));
    const float rho2 = pmax2 / (float)(n * n);
    // L = floor(256 log2 rho), 8.8 fixed point
    const uint32_t bits = __float_as_uint(rho2), ef = (bits >> 23) & 255u;
    const int lmax = 256 * ((int)mips - 1);
    int L = 0;
    if (ef == 255u) L = lmax;
    else if (ef != 0u) {
        const float m = __uint_as_float((bits & 0x007FFFFFu) | 0x3F800000u);
        uint32_t lo = 0u, hi = 127u;
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            const uint32_t mid = (lo + hi) >> 1;
            const bool ge = lo < hi && m >= lds[kLdsLod + min(mid, 126u)];
            if (lo < hi) { if (ge) lo = mid + 1u; else hi = mid; }
        }
        L = min(max(128 * ((int)ef - 127) + (int)lo, 0), lmax);
    }
    const uint32_t d = (uint32_t)L >> 8;
    // With SPLIT the gather comes in two forms, chosen by the wave as a whole: where no lane of the wave holds a BC format the levels are
    // read by the RGBA8 form, which has no format branch in it (the branch alone cost RGBA8 callers a tenth of the resolve's time); one BC
    // lane takes the whole wave through the mixed form. Without SPLIT there is the mixed form alone: the forward resolve has no registers
    // for both at three waves per SIMD
    const Lod lod = {d, (float)(L & 255) * 0.00390625f, n, ymajor ? dyu : dxu, ymajor ? dyv : dxv};
    if (SPLIT && __ballot(ur_bc::is_bc(format)) == 0ull) gather_levels<C0, N, false>(texels, width, height, mips, format, lod, u, v, lds, out);
    else gather_levels<C0, N, true>(texels, width, height, mips, format, lod, u, v, lds, out);
}

__device__ __forceinline__ bool valid_texture(const u32x4_t desc)
{
    const uint32_t format = (desc.w >> 8) & 0xFFu;
    const bool rgba8 = format == UR_TEXTURE_R8G8B8A8_UNORM || format == UR_TEXTURE_R8G8B8A8_UNORM_SRGB;
    const uint32_t align = rgba8 ? 4u : ur_bc::block_bytes(format); // 8 (BC1), 16 (BC3, BC5), 0: no format of the sampler
    return (desc.x | desc.y) != 0u && align != 0u && (desc.x & (align - 1u)) == 0u && (desc.z & 0xFFFFu) != 0u && (desc.z >> 16) != 0u && (desc.w & 0xFFu) != 0u;
}

} // namespace
