// The static sampler of the textured GBuffer resolve (DESIGN.md section 3.10 is its rule, tests/gbuffer_tex_ref.py the restatement):
// ApplyTextureTransform, wrap addressing, one bilinear sample, and the footprint / level of detail / trilinear probes of one map, as
// device inline functions over tables the including kernel has put into LDS (layout below). csrc/gbuffer_resolve.hip samples R, G and B
// with it, the masked raster's alpha test (csrc/raster.hip) channel A: the same sampler with another output.
#pragma once

#include "raster_rule.h"

#include "../../include/ur_raster.h"

namespace {

using ur_raster::u32x4_t;

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

// One bilinear sample of a level: the channels [C0, C0 + N) decoded through `tab` (LDS: the sRGB decode or code / 255)
template <int C0, int N>
__device__ __forceinline__ void bilinear(const uint32_t* __restrict__ level, uint32_t wd, uint32_t hd, float u, float v, const float* tab, float (&out)[N])
{
    uint32_t x0, x1, y0, y1;
    float fx, fy;
    wrap_pair(u, wd, x0, x1, fx);
    wrap_pair(v, hd, y0, y1, fy);
    const uint32_t* r0 = level + (size_t)y0 * wd;
    const uint32_t* r1 = level + (size_t)y1 * wd;
    const uint32_t t00 = r0[x0], t10 = r0[x1], t01 = r1[x0], t11 = r1[x1];
#pragma unroll
    for (int c = 0; c < N; ++c) {
        const float a = tab[(t00 >> (8 * (C0 + c))) & 255u], b = tab[(t10 >> (8 * (C0 + c))) & 255u];
        const float d = tab[(t01 >> (8 * (C0 + c))) & 255u], e = tab[(t11 >> (8 * (C0 + c))) & 255u];
        const float top = a + fx * (b - a), bottom = d + fx * (e - d);
        out[c] = top + fy * (bottom - top);
    }
}

// The static sampler on one map: footprint, level of detail, up to four trilinear probes. (u, v) the centre's coordinate, (dxu, dxv) and
// (dyu, dyv) the quad's differences; `desc` a valid descriptor's four dwords; `lds` the tables. The output is the channels [C0, C0 + N):
// R, G, B for a map of the resolve, A alone (C0 = 3: code / 255 whatever the format, and the decode table is not read) for the alpha test
template <int C0 = 0, int N = 3>
__device__ __forceinline__ void sample_map(const u32x4_t desc, float u, float v, float dxu, float dxv, float dyu, float dyv, const float* lds, float (&out)[N])
{
    const uint32_t* texels = reinterpret_cast<const uint32_t*>((uint64_t)desc.x | ((uint64_t)desc.y << 32));
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
    const float f = (float)(L & 255) * 0.00390625f;
    // a dimension is at most 65535, so every level from 16 on is 1 x 1: the shift count stays below the word's width for any `mips`
    size_t offset = 0u;
    for (uint32_t k = 0u; k < d; ++k) offset += (size_t)max(1u, width >> min(k, 16u)) * max(1u, height >> min(k, 16u));
    const uint32_t wd = max(1u, width >> min(d, 16u)), hd = max(1u, height >> min(d, 16u));
    const uint32_t d1 = min(d + 1u, mips - 1u);
    const uint32_t we = max(1u, width >> min(d1, 16u)), he = max(1u, height >> min(d1, 16u));
    const uint32_t* level0 = texels + offset;
    const uint32_t* level1 = d1 == d ? level0 : level0 + (size_t)wd * hd;
    const float* tab = lds + (C0 != 3 && format == UR_TEXTURE_R8G8B8A8_UNORM_SRGB ? kLdsDecode : kLdsUnorm);
    const float mu = ymajor ? dyu : dxu, mv = ymajor ? dyv : dxv;
    float sum[N] = {};
    for (uint32_t i = 0u; i < n; ++i) {
        const float o = kProbeOffset[n * (n - 1u) / 2u + i];
        const float pu = u + mu * o, pv = v + mv * o;
        float s[N];
        bilinear<C0, N>(level0, wd, hd, pu, pv, tab, s);
        if (f != 0.0f) { // (lo + 0 * (hi - lo) is lo: every value here is finite and no zero is negative)
            float t[N];
            bilinear<C0, N>(level1, we, he, pu, pv, tab, t);
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

__device__ __forceinline__ bool valid_texture(const u32x4_t desc)
{
    const uint32_t format = (desc.w >> 8) & 0xFFu;
    return (desc.x | desc.y) != 0u && (desc.x & 3u) == 0u && (desc.z & 0xFFFFu) != 0u && (desc.z >> 16) != 0u && (desc.w & 0xFFu) != 0u &&
           (format == UR_TEXTURE_R8G8B8A8_UNORM || format == UR_TEXTURE_R8G8B8A8_UNORM_SRGB);
}

} // namespace
