// Device functions of the post chain shared by csrc/tonemap.hip and csrc/post.hip: the Tonemap pixel (Shaders/Tonemap.hlsl)
// and the 8-bit rounding of the back buffer. ur_tonemap_cas must produce exactly ur_tonemap's bytes before it sharpens them,
// so there is one definition of each, compiled with the same flags (-ffp-contract=off) in both translation units. Not installed.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace ur_post {

typedef _Float16 half4_t __attribute__((ext_vector_type(4)));

struct TonemapParams {
    const half4_t* hdr;
    const float* exposure_ev; // LogAverageLuminance texel (0,0), nullable
    uint32_t* out;
    uint32_t count;
    uint32_t enable_tonemap, enable_auto_exposure;
    float exposure, inv_gamma;
};

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
