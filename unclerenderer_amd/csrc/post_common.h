// The post chain's one shared header (csrc/tonemap.hip, csrc/post.hip, csrc/taa.hip): the vector types and their bit casts, the Tonemap
// pixel (Shaders/Tonemap.hlsl) with the 8-bit rounding of the back buffer, and the one place its constants become launch parameters.
// ur_tonemap_cas and ur_temporal_aa_tonemap must produce exactly ur_tonemap's bytes, so there is one definition of each, compiled with
// the same flags (-ffp-contract=off) in the three translation units. Not installed.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/ur_hotpath.h"

namespace ur_post {

typedef _Float16 half4_t __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));

// two dwords as loaded are the eight bytes of an RGBA16F texel (every kernel loads and shifts dwords; only tonemap_pixel wants halves)
__device__ __forceinline__ half4_t as_half4(u32x2_t u) { return __builtin_bit_cast(half4_t, u); }

struct TonemapParams {
    const half4_t* hdr;
    const float* exposure_ev; // LogAverageLuminance texel (0,0), nullable
    uint32_t* out;
    uint32_t count;
    uint32_t enable_tonemap, enable_auto_exposure;
    float exposure, inv_gamma;
};

// ur_tonemap_constants as every launch that tonemaps takes them; hdr / count stay for ur_tonemap to set
inline TonemapParams tonemap_params(const ur_tonemap_constants* constants, const float* exposure_ev, uint32_t* out)
{
    TonemapParams p{};
    p.exposure_ev = exposure_ev;
    p.out = out;
    p.enable_tonemap = constants->EnableTonemap;
    p.enable_auto_exposure = constants->EnableAutoExposure;
    p.exposure = constants->Exposure;
    p.inv_gamma = 1.0f / (constants->Gamma > 1e-3f ? constants->Gamma : 1e-3f);
    return p;
}

__device__ __forceinline__ float pow_pos(float x, float e) { return x > 0.0f ? __builtin_amdgcn_exp2f(e * __builtin_amdgcn_logf(x)) : 0.0f; }
// saturate, then R8G8B8A8_UNORM rounding (round half up of x * 255)
__device__ __forceinline__ uint32_t unorm8(float x) { return (uint32_t)fmaf(fminf(fmaxf(x, 0.0f), 1.0f), 255.0f, 0.5f); }

// one pixel: RGBA16F -> packed R8G8B8A8 (Tonemap.hlsl:57-79)
__device__ __forceinline__ uint32_t tonemap_pixel(const TonemapParams& p, float finalExposure, half4_t h)
{
    {   // (block kept so that the body reads like the shader's main)
        float r = (float)h.x * finalExposure, g = (float)h.y * finalExposure, b = (float)h.z * finalExposure;
        if (p.enable_tonemap != 0) { // PBRNeutralToneMapping, Tonemap.hlsl:34-55
            const float startCompression = 0.8f - 0.04f, desaturation = 0.15f;
            const float x = fminf(r, fminf(g, b));
            const float offset = x < 0.08f ? fmaf(-6.25f * x, x, x) : 0.04f;
            r -= offset; g -= offset; b -= offset;
            const float peak = fmaxf(r, fmaxf(g, b));
            if (!(peak < startCompression)) {
                const float d = 1.0f - startCompression;
                // the three quotients through v_rcp_f32 (1 ulp): an IEEE divide is ~12 instructions each, which made this
                // stream VALU-bound; the 8-bit result moves by at most the one LSB the pow already allows
                const float newPeak = fmaf(-(d * d), __builtin_amdgcn_rcpf(peak + d - startCompression), 1.0f);
                const float s = newPeak * __builtin_amdgcn_rcpf(fmaxf(peak, 1e-4f));
                r *= s; g *= s; b *= s;
                const float gm = 1.0f - __builtin_amdgcn_rcpf(fmaf(desaturation, peak - newPeak, 1.0f));
                r = fmaf(gm, newPeak - r, r); g = fmaf(gm, newPeak - g, g); b = fmaf(gm, newPeak - b, b);
            }
        }
        r = fminf(fmaxf(r, 0.0f), 1.0f); g = fminf(fmaxf(g, 0.0f), 1.0f); b = fminf(fmaxf(b, 0.0f), 1.0f);
        r = pow_pos(r, p.inv_gamma); g = pow_pos(g, p.inv_gamma); b = pow_pos(b, p.inv_gamma);
        return unorm8(r) | (unorm8(g) << 8) | (unorm8(b) << 16) | 0xFF000000u;
    }
}

__device__ __forceinline__ float final_exposure(const TonemapParams& p)
{
    float e = p.exposure;
    if (p.enable_auto_exposure != 0 && p.exposure_ev != nullptr) e *= __builtin_amdgcn_exp2f(p.exposure_ev[0]);
    return e;
}

} // namespace ur_post
