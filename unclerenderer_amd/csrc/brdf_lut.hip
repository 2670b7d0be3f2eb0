// ur_brdf_lut (include/ur_brdf_lut.h): the split-sum BRDF table on the device, by the rule of csrc/brdf_lut_rule.h
// - the file the serial host build (csrc/brdf_lut_host.cpp) and tests/cpp/env_sky_main.cpp run. One launch, no scratch:
//   a wave a texel, four waves a workgroup; lane j adds its row's samples j, j + 64, ... (each one 16-byte load from the table), the
//   rule's tree over the wave follows and lane 0 stores the texel's four bytes.
// The kernel has C linkage: tests/test_env_panorama_abi.py pins the library's C++-mangled kernels, so a kernel added behind it carries a
// plain name. Built with -ffp-contract=off; every divide and square root is IEEE. Vector stores only.

#include "brdf_lut_rule.h"
#include "ur_internal.h"

#include "../../include/ur_brdf_lut.h"

namespace {
constexpr uint32_t kLutThreads = 256u;
constexpr uint32_t kLutWaves = kLutThreads / ur_lut::kLanes;
} // namespace

extern "C" __global__ __launch_bounds__(256) void ur_brdf_lut_kernel(ur_lut::Plan p, const ur_lut::Sample* __restrict__ table, uint32_t* __restrict__ dst)
{
    const uint32_t texel = blockIdx.x * kLutWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (texel >= p.texels) return; // (a whole wave)
    const ur_lut::Texel t = ur_lut::texel_of(p, texel);
    const ur_lut::Sample* samples = table + (size_t)t.row * p.samples;
    float sum[2] = {0.0f, 0.0f};
    for (uint32_t i = lane; i < p.samples; i += ur_lut::kLanes) ur_lut::add_sample(t, samples[i], sum);
#pragma unroll
    for (uint32_t stride = ur_lut::kLanes / 2u; stride != 0u; stride >>= 1) {
        sum[0] = sum[0] + __shfl_down(sum[0], stride, 64);
        sum[1] = sum[1] + __shfl_down(sum[1], stride, 64);
    }
    if (lane == 0u) dst[texel] = ur_lut::finish(sum, p.inv_samples);
}

extern "C" int ur_brdf_lut(ur_ctx* ctx, uint32_t width, uint32_t height, uint32_t sample_count, const void* table_device, size_t table_bytes, void* dst_device,
                           size_t dst_bytes)
{
    using namespace ur;
    if (!ctx) { set_error("ur_brdf_lut: null context"); return UR_EINVAL; }
    char text[256];
    if (ur_lut::refuse("ur_brdf_lut", width, height, sample_count, table_device, table_bytes, dst_device, dst_bytes, text, sizeof text)) {
        set_error("%s", text);
        return UR_EINVAL;
    }
    const ur_lut::Plan p = ur_lut::make_plan(width, height, sample_count);
    hipLaunchKernelGGL(ur_brdf_lut_kernel, dim3((p.texels + kLutWaves - 1u) / kLutWaves), dim3(kLutThreads), 0, ctx->stream, p,
                       static_cast<const ur_lut::Sample*>(table_device), static_cast<uint32_t*>(dst_device));
    UR_HIP_TRY(hipGetLastError());
    return UR_OK;
}
