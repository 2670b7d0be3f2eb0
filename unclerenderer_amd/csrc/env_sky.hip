// ur_env_sky (include/ur_env_sky.h): the procedural sky becomes the top level of an HDR cube on the device, by the
// rule of csrc/env_sky_rule.h - the file the serial host build (csrc/env_sky_host.cpp) and tests/cpp/env_sky_main.cpp run. One launch, no
// scratch, nothing read: the folded constants travel in the kernel's arguments.
//   a wave holds 64 / K^2 consecutive output texels when K^2 < 64 (K = 1: a lane a texel, 8-byte stores side by side) and one texel
//   otherwise; a lane adds its texel's taps lane, lane + 64, ..., the lanes of a texel meet in the tree's strides below K^2 - the strides
//   above would add the +0 of idle lanes - and the texel's first lane stores it.
// The kernel has C linkage: tests/test_env_panorama_abi.py pins the library's C++-mangled kernels, so a kernel added behind it carries a
// plain name and takes what a template would have taken as arguments.
// Built with -ffp-contract=off; every divide and square root is IEEE. Vector stores only.

#include "env_sky_rule.h"
#include "ur_internal.h"

#include "../../include/ur_env_sky.h"

namespace {
constexpr uint32_t kSkyThreads = 256u;
constexpr uint32_t kSkyWaves = kSkyThreads / ur_sky::kLanes;
} // namespace

extern "C" __global__ __launch_bounds__(256) void ur_env_sky_kernel(ur_sky::Plan p, uint64_t* __restrict__ dst)
{
    const uint32_t wave = blockIdx.x * kSkyWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    uint32_t texel, tap;
    ur_sky::lane_place(p, wave, lane, texel, tap);
    const uint32_t taps2 = 1u << p.taps2_log2;
    float sum[3] = {0.0f, 0.0f, 0.0f};
    if (texel < p.texels)
        for (uint32_t i = tap; i < taps2; i += ur_sky::kLanes) ur_sky::add_tap(p, texel, i, sum);
#pragma unroll
    for (uint32_t stride = ur_sky::kLanes / 2u; stride != 0u; stride >>= 1) {
        if (stride >= taps2) continue; // (the same in every lane)
#pragma unroll
        for (int c = 0; c < 3; ++c) sum[c] = sum[c] + __shfl_down(sum[c], stride, 64);
    }
    if (texel < p.texels && tap == 0u) dst[texel] = ur_sky::finish(sum, p.inv_taps2);
}

extern "C" int ur_env_sky(ur_ctx* ctx, const ur_sky_constants* sky, uint32_t base_size, uint32_t taps, void* dst_device, size_t dst_bytes)
{
    using namespace ur;
    if (!ctx) { set_error("ur_env_sky: null context"); return UR_EINVAL; }
    if (!sky) { set_error("ur_env_sky: null constants"); return UR_EINVAL; }
    char text[256];
    if (ur_sky::refuse("ur_env_sky", base_size, taps, dst_device, dst_bytes, text, sizeof text) ||
        ur_sky::refuse_constants("ur_env_sky", sky->CameraPosition, sky->LightDirection, sky->LightColor, text, sizeof text)) {
        set_error("%s", text);
        return UR_EINVAL;
    }
    const ur_sky::Plan p = ur_sky::make_plan(ur_sky::fold(sky->CameraPosition, sky->LightDirection, sky->LightColor), base_size, taps);
    hipLaunchKernelGGL(ur_env_sky_kernel, dim3((p.waves + kSkyWaves - 1u) / kSkyWaves), dim3(kSkyThreads), 0, ctx->stream, p, static_cast<uint64_t*>(dst_device));
    UR_HIP_TRY(hipGetLastError());
    return UR_OK;
}
