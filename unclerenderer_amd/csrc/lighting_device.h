// Device helpers that BOTH lighting kernels use (lighting.hip, lighting_tiled.hip), each defined once. What one kernel alone uses
// lives in that kernel's unit. Not installed.
#pragma once

#include "lighting_params.h"

namespace ur {

__device__ __forceinline__ float rcp(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ float rsq(float x) { return __builtin_amdgcn_rsqf(x); }
__device__ __forceinline__ float sat(float x) { return __builtin_amdgcn_fmed3f(x, 0.0f, 1.0f); }
__device__ __forceinline__ float mix(float a, float b, float t) { return fmaf(t, b - a, a); }

// base + 32-bit unsigned BYTE offset: lets the compiler use the SGPR-base + VGPR-offset addressing mode of global_load
// instead of 64-bit VALU address arithmetic (v_lshl_add_u64 per access).
// (The pointers are global memory by contract; saying so keeps pointers that were themselves loaded from memory off the
// flat_load path.)
#define UR_GLOBAL __attribute__((address_space(1)))
template <class T>
__device__ __forceinline__ T ld(const void* base, uint32_t byte_offset)
{
    return *reinterpret_cast<const UR_GLOBAL T*>((const UR_GLOBAL char*)base + byte_offset);
}
template <class T>
__device__ __forceinline__ void st(void* base, uint32_t byte_offset, T v)
{
    *reinterpret_cast<UR_GLOBAL T*>((UR_GLOBAL char*)base + byte_offset) = v;
}

struct uint4u { uint32_t x, y, z, w; };  // 16 bytes loaded from an 8-byte-aligned address
struct float3u { float x, y, z; };       // 12 bytes loaded from a 4-byte-aligned address
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
typedef float f32x3_t __attribute__((ext_vector_type(3)));
typedef u32x4_t u32x4_a8 __attribute__((aligned(8)));
typedef uint32_t u32x3_t __attribute__((ext_vector_type(3)));
typedef u32x3_t u32x3_a4 __attribute__((aligned(4)));
typedef f32x3_t f32x3_a4 __attribute__((aligned(4)));
template <>
__device__ __forceinline__ uint4u ld<uint4u>(const void* base, uint32_t byte_offset)
{
    const u32x4_t v = *reinterpret_cast<const UR_GLOBAL u32x4_a8*>((const UR_GLOBAL char*)base + byte_offset);
    return {v.x, v.y, v.z, v.w};
}
template <>
__device__ __forceinline__ float3u ld<float3u>(const void* base, uint32_t byte_offset)
{
    const f32x3_t v = *reinterpret_cast<const UR_GLOBAL f32x3_a4*>((const UR_GLOBAL char*)base + byte_offset);
    return {v.x, v.y, v.z};
}

struct F3 { float x, y, z; };
__device__ __forceinline__ F3 f3(float x, float y, float z) { return {x, y, z}; }
__device__ __forceinline__ float dot(F3 a, F3 b) { return fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)); }
__device__ __forceinline__ F3 mix(F3 a, F3 b, float t) { return {mix(a.x, b.x, t), mix(a.y, b.y, t), mix(a.z, b.z, t)}; }
// v * M for a row-major 3x3
__device__ __forceinline__ F3 rot(F3 v, const float* M)
{
    return f3(fmaf(v.z, M[6], fmaf(v.y, M[3], v.x * M[0])), fmaf(v.z, M[7], fmaf(v.y, M[4], v.x * M[1])),
              fmaf(v.z, M[8], fmaf(v.y, M[5], v.x * M[2])));
}

// acc += w * f16(lo/hi half of a packed dword): one mixed-precision FMA, no unpack/convert instructions
__device__ __forceinline__ float mix_lo(float acc, uint32_t packed, float w)
{
    asm("v_fma_mix_f32 %0, %1, %2, %0 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "+v"(acc) : "v"(packed), "v"(w));
    return acc;
}
__device__ __forceinline__ float mix_hi(float acc, uint32_t packed, float w)
{
    asm("v_fma_mix_f32 %0, %1, %2, %0 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(acc) : "v"(packed), "v"(w));
    return acc;
}
// the same without an addend (first tap of a sum: no zero-initialised accumulator register)
__device__ __forceinline__ float mul_lo(uint32_t packed, float w)
{
    float r;
    asm("v_fma_mix_f32 %0, %1, %2, 0 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(r) : "v"(packed), "v"(w));
    return r;
}
__device__ __forceinline__ float mul_hi(uint32_t packed, float w)
{
    float r;
    asm("v_fma_mix_f32 %0, %1, %2, 0 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r) : "v"(packed), "v"(w));
    return r;
}

// ---- gathers are split into "issue the loads" and "filter" so one pixel has every independent gather in flight
// before the BRDF math starts (the math hides their latency; no branch separates them) -----------------------------
struct CubeTaps { uint4u r0, r1; float fx, fy; };

// scale * bilinear(taps) [+ r when ACC]: 12 mixed-precision FMAs straight from the packed fp16 texels
template <bool ACC>
__device__ __forceinline__ void cube_taps_filter(F3& r, const CubeTaps& t, float scale)
{
    const float wy1 = t.fy * scale, wy0 = scale - wy1;
    const float w10 = wy0 * t.fx, w00 = wy0 - w10, w11 = wy1 * t.fx, w01 = wy1 - w11;
    const float x0 = ACC ? mix_lo(r.x, t.r0.x, w00) : mul_lo(t.r0.x, w00);
    const float y0 = ACC ? mix_hi(r.y, t.r0.x, w00) : mul_hi(t.r0.x, w00);
    const float z0 = ACC ? mix_lo(r.z, t.r0.y, w00) : mul_lo(t.r0.y, w00);
    r.x = mix_lo(mix_lo(mix_lo(x0, t.r0.z, w10), t.r1.x, w01), t.r1.z, w11);
    r.y = mix_hi(mix_hi(mix_hi(y0, t.r0.z, w10), t.r1.x, w01), t.r1.z, w11);
    r.z = mix_lo(mix_lo(mix_lo(z0, t.r0.w, w10), t.r1.y, w01), t.r1.w, w11);
}

// SkyAtmosphere.hlsl:58-93 with the camera-height densities, phase constants and sun attenuation folded on the host.
// P: pointer to the parameters (generic for the per-tile kernel; a re-read kernarg pointer in the streaming kernel)
template <class P>
__device__ __forceinline__ F3 sky_pixel(P p, float vx, float vy)
{
    const auto* Q = p->skyRot;
    F3 w = f3(fmaf(vy, Q[1], fmaf(vx, Q[0], Q[2])), fmaf(vy, Q[4], fmaf(vx, Q[3], Q[5])), fmaf(vy, Q[7], fmaf(vx, Q[6], Q[8])));
    const float wr = rsq(dot(w, w));
    w = f3(w.x * wr, w.y * wr, w.z * wr);
    const float h = 1.0f - sat(fmaf(w.y, 0.5f, 0.5f));
    const float falloff = sat(h * h * h);
    const float cosSunView = dot(w, f3(p->sunDir[0], p->sunDir[1], p->sunDir[2]));
    const float rayleighPhase = fmaf(cosSunView, cosSunView, 1.0f);
    const float g = 0.76f, g2 = g * g;
    const float mb = fmaf(-2.0f * g, cosSunView, 1.0f + g2);
    const float denom = mb * __builtin_amdgcn_sqrtf(mb); // pow(x, 1.5)
    const float miePhase = rcp(fmaxf(denom, 1e-3f));
    F3 c;
    c.x = fmaf(fmaf(p->skyMie[0], miePhase, p->skyScatterR[0] * rayleighPhase), p->sunAttenuation, mix(0.05f, 0.52f, falloff));
    c.y = fmaf(fmaf(p->skyMie[1], miePhase, p->skyScatterR[1] * rayleighPhase), p->sunAttenuation, mix(0.12f, 0.68f, falloff));
    c.z = fmaf(fmaf(p->skyMie[2], miePhase, p->skyScatterR[2] * rayleighPhase), p->sunAttenuation, mix(0.22f, 0.86f, falloff));
    return c;
}

} // namespace ur
