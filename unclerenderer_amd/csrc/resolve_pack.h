// What the two resolves over the visibility keys (csrc/gbuffer_resolve.hip, csrc/forward_resolve.hip) share beside visibility_key.h and gbuffer_interp.h: the
// 4-byte aligned load of 16 bytes of a vertex and the RGBA16F store's packing. Device inline functions only.
#pragma once

#include "ur_device.h"

namespace ur_raster {

typedef float f32x4u_t __attribute__((ext_vector_type(4), aligned(4))); // 16 bytes of a vertex: 4-byte aligned

__device__ __forceinline__ uint32_t half_bits(float v)
{
    const _Float16 h = (_Float16)v; // round to nearest even
    return (uint32_t)__builtin_bit_cast(unsigned short, h);
}
__device__ __forceinline__ ur::once_u32x2_t pack_half4(float x, float y, float z, float w)
{
    return ur::once_u32x2_t{half_bits(x) | (half_bits(y) << 16), half_bits(z) | (half_bits(w) << 16)};
}

} // namespace ur_raster
