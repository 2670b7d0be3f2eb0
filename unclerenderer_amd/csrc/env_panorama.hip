// ur_env_panorama (include/ur_env_panorama.h): the RGBE texels of a lat-long panorama become the top level of an
// HDR cube on the device, by the rule of csrc/env_panorama_rule.h - the file the serial host build (csrc/env_panorama_host.cpp) and
// tests/cpp/env_panorama_main.cpp run. One launch, no scratch:
//   a wave holds 64 / K^2 consecutive output texels when K^2 < 64 (K = 1: a lane a texel, 8-byte stores side by side) and one texel
//   otherwise; a lane adds its texel's taps lane, lane + 64, ... (each one bilinear sample: four 4-byte gathers from the panorama), the
//   lanes of a texel meet in the tree's strides below K^2 - the strides above would add the +0 of idle lanes - and the texel's first lane
//   stores it.
// Built with -ffp-contract=off; every divide and square root is IEEE. Vector stores only.

#include "env_panorama_rule.h"
#include "ur_internal.h"

#include "../../include/ur_env_panorama.h"

namespace ur {
namespace {

constexpr uint32_t kThreads = 256u;
constexpr uint32_t kWaves = kThreads / ur_pano::kLanes;

__global__ __launch_bounds__(kThreads) void panorama_cube_kernel(ur_pano::Plan p, const uint32_t* __restrict__ rgbe, uint64_t* __restrict__ dst)
{
    const uint32_t wave = blockIdx.x * kWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    uint32_t texel, tap;
    ur_pano::lane_place(p, wave, lane, texel, tap);
    const uint32_t taps2 = 1u << p.taps2_log2;
    float sum[3] = {0.0f, 0.0f, 0.0f};
    if (texel < p.texels)
        for (uint32_t i = tap; i < taps2; i += ur_pano::kLanes) ur_pano::add_tap(p, rgbe, texel, i, sum);
#pragma unroll
    for (uint32_t stride = ur_pano::kLanes / 2u; stride != 0u; stride >>= 1) {
        if (stride >= taps2) continue; // (the same in every lane)
#pragma unroll
        for (int c = 0; c < 3; ++c) sum[c] = sum[c] + __shfl_down(sum[c], stride, 64);
    }
    if (texel < p.texels && tap == 0u) dst[texel] = ur_pano::finish(sum, p.inv_taps2);
}

} // namespace
} // namespace ur

extern "C" int ur_env_panorama(ur_ctx* ctx, const void* rgbe_device, size_t rgbe_bytes, uint32_t width, uint32_t height, uint32_t base_size, uint32_t taps,
                               void* dst_device, size_t dst_bytes)
{
    using namespace ur;
    if (!ctx) { set_error("ur_env_panorama: null context"); return UR_EINVAL; }
    char text[256];
    if (ur_pano::refuse("ur_env_panorama", rgbe_device, rgbe_bytes, width, height, base_size, taps, dst_device, dst_bytes, text, sizeof text)) {
        set_error("%s", text);
        return UR_EINVAL;
    }
    const ur_pano::Plan p = ur_pano::make_plan(width, height, base_size, taps);
    hipLaunchKernelGGL(panorama_cube_kernel, dim3((p.waves + kWaves - 1u) / kWaves), dim3(kThreads), 0, ctx->stream, p, static_cast<const uint32_t*>(rgbe_device),
                       static_cast<uint64_t*>(dst_device));
    UR_HIP_TRY(hipGetLastError());
    return UR_OK;
}
