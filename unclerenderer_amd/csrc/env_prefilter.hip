// ur_env_prefilter (include/ur_env_prefilter.h): the top level of an HDR cube becomes the prefiltered chain on the
// device, by the rule of csrc/env_prefilter_rule.h - the file the serial host build (csrc/env_prefilter_host.cpp) and
// tests/cpp/env_prefilter_main.cpp run. At most L + 3 launches, each reading only what the one in front of it has finished writing:
//   top     a lane one texel of level 0: into the destination and into the pyramid (scratch).
//   down    one launch a pyramid level, a lane one texel: the 2 x 2 box mean of the level above.
//   stage   ur_env_cube_build's decode and border launches (launch_env_cube_bordered) over the pyramid: bordered faces, in scratch.
//   filter  every level 1 .. L - 1 in one launch. A workgroup takes kGroupTexels consecutive texels of one level and copies that level's
//           samples (16 bytes each, at most 64 KiB) into LDS once; a wave takes four of the texels, one after the other: lane j adds
//           the samples j, j + 64, ... (each one trilinear sample: eight 8-byte gathers from the bordered pyramid), the lanes' sums
//           meet in a fixed tree by strides 32 .. 1, and lane 0 stores the texel. A lane a texel would leave the small levels as one
//           serial chain of S dependent gathers; this way the 6-texel level is 6 waves of S / 64 steps.
// Built with -ffp-contract=off; every divide and square root is IEEE. Vector stores only.

#include "env_prefilter_rule.h"
#include "ur_internal.h"

#include "../../include/ur_env_prefilter.h"

namespace ur {
namespace {

constexpr uint32_t kThreads = 256u;
constexpr uint32_t kWaveTexels = ur_envp::kGroupTexels / (kThreads / 64u);

__global__ __launch_bounds__(kThreads) void env_bake_top_kernel(ur_envp::Plan p, const uint64_t* __restrict__ src, uint64_t* __restrict__ dst, uint64_t* __restrict__ pyramid)
{
    const uint32_t item = blockIdx.x * kThreads + threadIdx.x;
    if (item >= 6u * p.base * p.base) return;
    ur_envp::top_item(p, src, dst, pyramid, item);
}

__global__ __launch_bounds__(kThreads) void env_bake_down_kernel(ur_envp::Plan p, uint64_t* pyramid, uint32_t m)
{
    const uint32_t item = blockIdx.x * kThreads + threadIdx.x, n = p.base >> m;
    if (item >= 6u * n * n) return;
    ur_envp::down_item(p, pyramid, m, item);
}

__global__ __launch_bounds__(kThreads) void env_bake_filter_kernel(ur_envp::Plan p, const uint64_t* __restrict__ staged, const float4* __restrict__ table,
                                                                   uint64_t* __restrict__ dst)
{
    extern __shared__ float4 samples[]; // the level's p.samples entries
    const uint32_t group = blockIdx.x;  // (the same in every lane, as is everything derived from it)
    const uint32_t k = ur_envc::level_of(p.group_start, group);
    const float4* level = table + p.levels + (size_t)(k - 1u) * p.samples;
    for (uint32_t i = threadIdx.x; i < p.samples; i += kThreads) samples[i] = level[i];
    const float inv_weight = table[k].x;
    __syncthreads();
    const uint32_t n = p.base >> k, texels = 6u * n * n, lane = threadIdx.x & 63u;
    const uint32_t first = (group - ur_envc::at32(p.group_start, k)) * ur_envp::kGroupTexels + (threadIdx.x >> 6) * kWaveTexels;
    for (uint32_t w = 0u; w < kWaveTexels; ++w) {
        const uint32_t t = first + w;
        if (t >= texels) break; // (a whole wave at once)
        const ur_envp::Place o = ur_envp::place_of(p, k, t);
        const ur_envp::Frame f = ur_envp::texel_frame(o.face, o.x, o.y, o.n);
        float sum[3] = {0.0f, 0.0f, 0.0f};
        for (uint32_t i = lane; i < p.samples; i += ur_envp::kLanes) {
            const float4 e = samples[i];
            if (e.z > 0.0f) ur_envp::add_sample(p, staged, f, ur_envp::Sample{e.x, e.y, e.z, e.w}, sum);
        }
#pragma unroll
        for (uint32_t stride = ur_envp::kLanes / 2u; stride != 0u; stride >>= 1) {
#pragma unroll
            for (int c = 0; c < 3; ++c) sum[c] = sum[c] + __shfl_down(sum[c], stride, 64);
        }
        if (lane == 0u) dst[o.at] = ur_envp::finish(sum, inv_weight);
    }
}

uint32_t groups(uint32_t items) { return (items + kThreads - 1u) / kThreads; }

} // namespace
} // namespace ur

extern "C" int ur_env_prefilter(ur_ctx* ctx, const void* src_device, size_t src_bytes, uint32_t base_size, uint32_t sample_count, const void* table_device,
                                size_t table_bytes, void* dst_device, size_t dst_bytes, void* scratch, size_t scratch_bytes)
{
    using namespace ur;
    if (!ctx) { set_error("ur_env_prefilter: null context"); return UR_EINVAL; }
    char text[256];
    if (ur_envp::refuse("ur_env_prefilter", src_device, src_bytes, base_size, sample_count, table_device, table_bytes, dst_device, dst_bytes, scratch, scratch_bytes,
                        true, text, sizeof text)) {
        set_error("%s", text);
        return UR_EINVAL;
    }
    const ur_envp::Plan p = ur_envp::make_plan(base_size, sample_count);
    uint64_t* dst = static_cast<uint64_t*>(dst_device);
    uint64_t* pyramid = static_cast<uint64_t*>(scratch);
    uint64_t* staged = pyramid + ur_envp::payload_bytes(base_size) / 8u;
    const dim3 threads(kThreads);
    hipLaunchKernelGGL(env_bake_top_kernel, dim3(groups(6u * base_size * base_size)), threads, 0, ctx->stream, p, static_cast<const uint64_t*>(src_device), dst, pyramid);
    for (uint32_t m = 1u; m < p.levels; ++m)
        hipLaunchKernelGGL(env_bake_down_kernel, dim3(groups(6u * (base_size >> m) * (base_size >> m))), threads, 0, ctx->stream, p, pyramid, m);
    if (p.levels > 1u) {
        launch_env_cube_bordered(ctx->stream, ur_envc::make_plan(ur_envc::kRGBA16F, base_size, p.levels), pyramid, staged);
        hipLaunchKernelGGL(env_bake_filter_kernel, dim3(p.groups), threads, 16u * sample_count, ctx->stream, p, staged, static_cast<const float4*>(table_device), dst);
    }
    UR_HIP_TRY(hipGetLastError());
    return UR_OK;
}
