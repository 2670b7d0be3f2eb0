// ur_env_cube_build (include/ur_env_cube.h): a DDS cube payload becomes the staged environment cube on the device,
// by the rule of csrc/env_cube_rule.h over the decoder of csrc/bc6h_decode.h - the files the serial host build (csrc/env_cube_host.cpp) and
// tests/cpp/env_cube_main.cpp run. Three launches, whatever the mip count, no scratch buffer; a lane is one item of the rule:
//   decode  reads the payload, writes the interior of every bordered face. A lane is one texel row of one block: it loads its block (16
//           bytes; the four lanes of a block load the same bytes), decodes the header and stores the row's texels, up to 32 consecutive
//           bytes; a level's items run block column first, so a wave's stores cover consecutive bytes of a texel row. The BC6H tables
//           (160 bytes) are staged from __constant__ memory into LDS once per workgroup: they are read under a lane's own index.
//           Lane 0 of the launch clears the info word.
//   border  reads interior texels (what decode wrote), writes the one-texel ring of every face (what decode did not). Its lanes also
//           count the reserved-mode blocks, one block's first byte a lane, and add a wave's count to the info word - one atomic add a
//           wave, and none when the wave met no such block, as in every cube a compressor wrote.
//   pairs   reads the bordered section, writes the row-pair section: a lane one 12-byte entry, neighbouring lanes neighbouring entries.
// A launch reads only what the launch in front of it has finished writing. Vector stores and one vector atomic only.

#include "env_cube_rule.h"
#include "ur_internal.h"

namespace ur {
namespace {

constexpr uint32_t kThreads = 256u;

__constant__ ur_bc6h::Tables g_bc6h_tables = ur_bc6h::kTables;

template <uint32_t FORMAT>
__global__ __launch_bounds__(kThreads) void env_cube_decode_kernel(ur_envc::Plan p, const void* src, uint64_t* dst, uint32_t* info)
{
    constexpr bool kBc6h = FORMAT != ur_envc::kRGBA16F;
    __shared__ ur_bc6h::Tables tables;
    if constexpr (kBc6h) {
        if (threadIdx.x < sizeof(ur_bc6h::Tables) / 4u)
            reinterpret_cast<uint32_t*>(&tables)[threadIdx.x] = reinterpret_cast<const uint32_t*>(&g_bc6h_tables)[threadIdx.x];
        __syncthreads();
    }
    const uint32_t item = blockIdx.x * kThreads + threadIdx.x;
    if (item == 0u && info) info[0] = 0u;
    if (item >= 6u * p.decode_face) return;
    ur_envc::decode_item(p, src, dst, item, kBc6h, FORMAT == ur_envc::kSF16, &tables);
}

__global__ __launch_bounds__(kThreads) void env_cube_border_kernel(ur_envc::Plan p, const void* src, uint64_t* dst, uint32_t* info)
{
    const uint32_t item = blockIdx.x * kThreads + threadIdx.x;
    if (info && p.total_blocks != 0u) { // (the same in every lane)
        const bool reserved = item < p.total_blocks && ur_bc6h::reserved_mode(static_cast<const uint32_t*>(src)[4u * (size_t)item]);
        const uint32_t count = (uint32_t)__popcll(__ballot(reserved));
        if (count != 0u && (threadIdx.x & 63u) == 0u) atomicAdd(info, count);
    }
    if (item >= 6u * p.border_face) return;
    ur_envc::border_item(p, dst, item);
}

__global__ __launch_bounds__(kThreads) void env_cube_pairs_kernel(ur_envc::Plan p, uint64_t* dst)
{
    const uint32_t item = blockIdx.x * kThreads + threadIdx.x;
    if (item >= 6u * p.pair_face) return;
    ur_envc::pair_item(p, dst, item);
}

uint32_t groups(uint32_t items) { return (items + kThreads - 1u) / kThreads; }

} // namespace

// The decode and border launches over an RGBA16F payload, no info word: the bordered section alone (the environment prefilter stages
// its source pyramid with them, csrc/env_prefilter.hip). The caller has checked the arguments and looks at hipGetLastError.
void launch_env_cube_bordered(hipStream_t stream, const ur_envc::Plan& p, const void* src, uint64_t* dst)
{
    const dim3 threads(kThreads);
    hipLaunchKernelGGL(env_cube_decode_kernel<ur_envc::kRGBA16F>, dim3(groups(6u * p.decode_face)), threads, 0, stream, p, src, dst, (uint32_t*)nullptr);
    hipLaunchKernelGGL(env_cube_border_kernel, dim3(groups(6u * p.border_face)), threads, 0, stream, p, src, dst, (uint32_t*)nullptr);
}

} // namespace ur

extern "C" int ur_env_cube_build(ur_ctx* ctx, const void* src_device, size_t src_bytes, uint32_t format, uint32_t base_size, uint32_t mip_count,
                                 ur_half4* dst_device, size_t dst_texels, uint32_t* info_device)
{
    using namespace ur;
    if (!ctx) { set_error("ur_env_cube_build: null context"); return UR_EINVAL; }
    char text[256];
    if (ur_envc::refuse("ur_env_cube_build", src_device, src_bytes, format, base_size, mip_count, dst_device, dst_texels, info_device, text, sizeof text)) {
        set_error("%s", text);
        return UR_EINVAL;
    }
    const ur_envc::Plan p = ur_envc::make_plan(format, base_size, mip_count);
    uint64_t* dst = reinterpret_cast<uint64_t*>(dst_device);
    const dim3 decode(groups(6u * p.decode_face)), threads(kThreads);
    if (format == ur_envc::kSF16) hipLaunchKernelGGL(env_cube_decode_kernel<ur_envc::kSF16>, decode, threads, 0, ctx->stream, p, src_device, dst, info_device);
    else if (format == ur_envc::kUF16) hipLaunchKernelGGL(env_cube_decode_kernel<ur_envc::kUF16>, decode, threads, 0, ctx->stream, p, src_device, dst, info_device);
    else hipLaunchKernelGGL(env_cube_decode_kernel<ur_envc::kRGBA16F>, decode, threads, 0, ctx->stream, p, src_device, dst, info_device);
    const uint32_t border_items = 6u * p.border_face, counted = info_device ? p.total_blocks : 0u;
    hipLaunchKernelGGL(env_cube_border_kernel, dim3(groups(border_items > counted ? border_items : counted)), threads, 0, ctx->stream, p, src_device, dst, info_device);
    hipLaunchKernelGGL(env_cube_pairs_kernel, dim3(groups(6u * p.pair_face)), threads, 0, ctx->stream, p, dst);
    UR_HIP_TRY(hipGetLastError());
    return UR_OK;
}
