// What the raster (csrc/raster_front.h, csrc/raster_kernels.h) and GBuffer's resolve (csrc/gbuffer_resolve.hip) must compute alike to decide a texel alike - not
// constants only: the launch shape, the finite test's bound, the depth passes' guard band, and as device functions rule 4's tie-break
//  and the near clip's select (section 3.8). The host checks' alignment test rides along. Nothing else belongs here.
#pragma once

#include <hip/hip_runtime.h>

namespace ur_raster {

typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));

constexpr uint32_t kThreads = 256u, kWaves = kThreads / 64u;
constexpr float kFloatMax = 3.402823466e38f;
constexpr float kDepthGuardBand = 2097152.0f; // 2^21 px: snapped coordinates below 2^29, edge functions exact in 64 bits

// Rule 4's tie-break as a bias: the edge a->b passes iff E - bias >= 0, bias 0 on a top (dy == 0 && dx > 0) or left (dy < 0) edge
__device__ __forceinline__ int edge_bias(int ax, int ay, int bx, int by)
{
    const int dx = bx - ax, dy = by - ay;
    return (dy < 0 || (dy == 0 && dx > 0)) ? 0 : 1;
}

__device__ __forceinline__ float sel3(uint32_t r, float u0, float u1, float u2) { return r == 0u ? u0 : (r == 1u ? u1 : u2); }

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1u)) == 0u; }

} // namespace ur_raster
