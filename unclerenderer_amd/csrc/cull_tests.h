// The three visibility tests of CullIndirectArgs (cull_kernels.h), each a statement-by-statement restatement of the reference:
// IsAabbVisible and IsOccluded of Shaders/CullIndirectArgs.hlsl:24-167 for the camera, RendererUtils::IsAabbInCameraFrustum for the
// extra views. Compiled with -ffp-contract=off and IEEE division, so every intermediate equals the oracle's.
#pragma once

#include "cull_params.h"

namespace {

__device__ __forceinline__ float saturate_f(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }
__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

__device__ __forceinline__ bool IsAabbVisible(const CullParams& C, float3 mn, float3 mx)
{
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const float4 plane = C.FrustumPlanes[i];
        const float px = plane.x >= 0.0f ? mx.x : mn.x;
        const float py = plane.y >= 0.0f ? mx.y : mn.y;
        const float pz = plane.z >= 0.0f ? mx.z : mn.z;
        if (dot3(plane.x, plane.y, plane.z, px, py, pz) + plane.w < 0.0f) return false;
    }
    return true;
}

// RendererUtils::IsAabbInCameraFrustum (RendererUtils.cpp:1192-1218) as oracle/ur_oracle.cpp restates it - the test of the reference's
// CPU visibility loops, kept apart from IsAabbVisible: a plane component >= 0 (-0 included, NaN not) picks max, d is summed in this
// order without contraction, and only d < 0 rejects (a NaN d, the camera's plane 4 under the reverse-Z infinite projection, never does)
__device__ __forceinline__ bool IsAabbInCameraFrustum(const float4* planes, float4 bmin, float4 bmax)
{
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const float4 P = planes[i];
        const float X = P.x >= 0.0f ? bmax.x : bmin.x;
        const float Y = P.y >= 0.0f ? bmax.y : bmin.y;
        const float Z = P.z >= 0.0f ? bmax.z : bmin.z;
        const float d = ((P.x * X + P.y * Y) + P.z * Z) + P.w * 1.0f;
        if (d < 0.0f) return false;
    }
    return true;
}

__device__ __forceinline__ bool IsOccluded(const CullParams& C, float3 mn, float3 mx)
{
    if (C.HZBEnabled == 0 || C.HZBWidth == 0 || C.HZBHeight == 0 || C.HZBMipCount == 0) return false;
    const float* M = C.ViewProjection;
    float minUx = 1.0f, minUy = 1.0f, maxUx = 0.0f, maxUy = 0.0f, maxDepth = 0.0f;
    bool anyBehind = false;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float cx = (i & 1) ? mx.x : mn.x, cy = (i & 2) ? mx.y : mn.y, cz = (i & 4) ? mx.z : mn.z;
        const float clx = ((cx * M[0] + cy * M[4]) + cz * M[8]) + 1.0f * M[12];
        const float cly = ((cx * M[1] + cy * M[5]) + cz * M[9]) + 1.0f * M[13];
        const float clz = ((cx * M[2] + cy * M[6]) + cz * M[10]) + 1.0f * M[14];
        const float clw = ((cx * M[3] + cy * M[7]) + cz * M[11]) + 1.0f * M[15];
        if (clw <= 0.0f) anyBehind = true; // the HLSL breaks out here; nothing after the break feeds the result
        const float nx = clx / clw, ny = cly / clw, nz = clz / clw;
        const float ux = nx * 0.5f + 0.5f;
        const float uy = 1 - (ny * 0.5f + 0.5f);
        minUx = fminf(minUx, ux); minUy = fminf(minUy, uy);
        maxUx = fmaxf(maxUx, ux); maxUy = fmaxf(maxUy, uy);
        maxDepth = fmaxf(maxDepth, nz);
    }
    if (anyBehind) return false;
    if (maxUx < 0.0f || maxUy < 0.0f || minUx > 1.0f || minUy > 1.0f) return false;
    minUx = saturate_f(minUx); minUy = saturate_f(minUy);
    maxUx = saturate_f(maxUx); maxUy = saturate_f(maxUy);
    const float ex = maxUx - minUx, ey = maxUy - minUy;
    const float psx = ex * (float)C.HZBWidth, psy = ey * (float)C.HZBHeight;
    const float maxDim = fmaxf(psx, psy);
    uint32_t mipLevel = 0;
    if (maxDim > 1.0f) {
        const uint32_t e = ((__float_as_uint(maxDim) >> 23) & 0xFFu) - 127u; // floor(log2(maxDim)), exact
        const float l = fminf(fmaxf((float)e, 0.0f), (float)(C.HZBMipCount - 1u));
        mipLevel = (uint32_t)l;
    }
    const uint32_t mipWidth = max(1u, C.HZBWidth >> mipLevel);
    const uint32_t mipHeight = max(1u, C.HZBHeight >> mipLevel);
    uint32_t minX = (uint32_t)(minUx * (float)mipWidth), minY = (uint32_t)(minUy * (float)mipHeight);
    uint32_t maxX = (uint32_t)(maxUx * (float)mipWidth), maxY = (uint32_t)(maxUy * (float)mipHeight);
    minX = min(minX, mipWidth - 1u); minY = min(minY, mipHeight - 1u);
    maxX = min(maxX, mipWidth - 1u); maxY = min(maxY, mipHeight - 1u);
    const float* mip = C.hzb + C.mip_offset[mipLevel];
    const uint32_t pitch = C.mip_width[mipLevel];
    // HLSL min ignores a NaN texel, signalling or quiet: the loads are quieted first (a raw sNaN operand of v_min_f32 gives NaN)
    float hzbDepth = 1.0f;
    hzbDepth = fminf(hzbDepth, __builtin_canonicalizef(mip[(size_t)minY * pitch + minX]));
    hzbDepth = fminf(hzbDepth, __builtin_canonicalizef(mip[(size_t)minY * pitch + maxX]));
    hzbDepth = fminf(hzbDepth, __builtin_canonicalizef(mip[(size_t)maxY * pitch + minX]));
    hzbDepth = fminf(hzbDepth, __builtin_canonicalizef(mip[(size_t)maxY * pitch + maxX]));
    return maxDepth < hzbDepth;
}

} // namespace
