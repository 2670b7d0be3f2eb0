// ur_texture_transcode (include/ur_raster.h): a chain of BC1 / BC2 / BC3 / BC4 / BC5 / BC7 levels becomes
// ur_texture2d's RGBA8 chain, in one launch whatever the number of levels. The decode is csrc/bc_wide_decode.h, the file the host
// decoder (csrc/bc_host.cpp) runs.
//
// A work item is one row of one block: a lane loads its block once (8 or 16 bytes), decodes the row's four texels and stores them - as
// one 16-byte store where all four lie inside the level and the address is 16-byte aligned, as dword stores otherwise (`rgba8` is only
// 4-byte aligned, and a level of odd width moves every row). Within a level, item j is texel row j / across and block column
// j % across, so neighbouring lanes write neighbouring 16 bytes of one texel row. Four lanes, a block row of items apart, read the
// same block: the loads are plain, the stores nontemporal (written once, read by later launches: DESIGN.md 3.3).
// The at most 17 distinct level sizes (levels 0..15, and the one-block levels from 16 on as one run) are a table in the arguments.

#include "bc_wide_decode.h"
#include "ur_internal.h"

namespace ur {
namespace {

constexpr uint32_t kThreads = 256, kLevels = 17;

struct TranscodeParams {
    const uint8_t* src;
    uint32_t* dst;
    uint32_t width, height, total; // total: work items of the whole chain
    uint32_t start[kLevels];       // the first work item of level l; entry 16 is the run of levels 16.., one item each; `total` where the chain ends before l
    uint32_t src_block[kLevels];   // blocks in front of level l
    uint64_t dst_texel[kLevels];   // texels in front of level l
};

typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));

__constant__ ur_bc::WideTables g_wide_tables = ur_bc::kWideTables;

// the level that holds `item`, what lies in front of it, and the first item of the level behind it
struct LevelAt { uint32_t level, start, next, src_block; uint64_t dst_texel; };
__device__ __forceinline__ LevelAt level_of(const TranscodeParams& p, uint32_t item)
{
    LevelAt at = {0u, 0u, p.total, 0u, 0u};
#pragma unroll
    for (uint32_t l = kLevels - 1u; l >= 1u; --l) { // downwards: `next` ends as the lowest start above the item
        const bool in = item >= p.start[l];
        at.next = in ? at.next : p.start[l];
        if (in && at.level == 0u) { at.level = l; at.start = p.start[l]; at.src_block = p.src_block[l]; at.dst_texel = p.dst_texel[l]; }
    }
    return at;
}

template <uint32_t FORMAT>
__global__ __launch_bounds__(kThreads) void texture_transcode_kernel(TranscodeParams p)
{
    __shared__ ur_bc::WideTables tables; // BC7 alone indexes them
    if constexpr (FORMAT == ur_bc::kBC7) {
        if (threadIdx.x < sizeof(ur_bc::WideTables) / 4u)
            reinterpret_cast<uint32_t*>(&tables)[threadIdx.x] = reinterpret_cast<const uint32_t*>(&g_wide_tables)[threadIdx.x];
        __syncthreads();
    }
    const uint32_t item = blockIdx.x * kThreads + threadIdx.x;
    if (item >= p.total) return;
    // the item's level. A wave's 64 items are consecutive, so nearly every wave lies inside one level: the table is searched once for the
    // wave's first item, in scalar registers, and per lane (selects, no array under a lane's index) only by a wave that straddles two levels
    const uint32_t first = __builtin_amdgcn_readfirstlane(item);
    LevelAt at = level_of(p, first);
    if (first + 63u >= at.next) at = level_of(p, item);
    const uint32_t level = at.level, start = at.start, src_block = at.src_block;
    const uint64_t dst_texel = at.dst_texel;
    const bool run = level == 16u; // one block, one texel a level: item j is level 16 + j
    const uint32_t j = item - start;
    const uint32_t wk = ur_bc::level_size(p.width, level), across = ur_bc::blocks_across(wk);
    const uint32_t y = run ? 0u : j / across, bx = run ? 0u : j - y * across;
    const uint32_t block = src_block + (run ? j : (y >> 2) * across + bx);
    constexpr uint32_t kBytes = FORMAT == ur_bc::kBC1 || FORMAT == ur_bc::kBC4 ? 8u : 16u;
    uint64_t lo, hi = 0u;
    if constexpr (kBytes == 8u) {
        const u32x2_t b = *reinterpret_cast<const u32x2_t*>(p.src + (size_t)block * 8u);
        lo = (uint64_t)b.x | ((uint64_t)b.y << 32);
    } else {
        const u32x4_t b = *reinterpret_cast<const u32x4_t*>(p.src + (size_t)block * 16u);
        lo = (uint64_t)b.x | ((uint64_t)b.y << 32);
        hi = (uint64_t)b.z | ((uint64_t)b.w << 32);
    }
    const uint32_t n = 4u * (y & 3u);
    u32x4_t row;
    row.x = ur_bc::source_word(FORMAT, lo, hi, n, &tables);
    row.y = ur_bc::source_word(FORMAT, lo, hi, n + 1u, &tables);
    row.z = ur_bc::source_word(FORMAT, lo, hi, n + 2u, &tables);
    row.w = ur_bc::source_word(FORMAT, lo, hi, n + 3u, &tables);
    const uint32_t inside = wk - 4u * bx; // texels of this block row inside the level (4 or more: all four)
    uint32_t* out = p.dst + (dst_texel + (run ? (uint64_t)j : (uint64_t)y * wk + 4u * bx));
    if (inside >= 4u && (reinterpret_cast<uintptr_t>(out) & 15u) == 0u) {
        __builtin_nontemporal_store(row, reinterpret_cast<u32x4_t*>(out));
    } else {
        __builtin_nontemporal_store(row.x, out);
        if (inside > 1u) __builtin_nontemporal_store(row.y, out + 1);
        if (inside > 2u) __builtin_nontemporal_store(row.z, out + 2);
        if (inside > 3u) __builtin_nontemporal_store(row.w, out + 3);
    }
}

template <uint32_t FORMAT>
int launch(ur_ctx* ctx, const TranscodeParams& p)
{
    hipLaunchKernelGGL(texture_transcode_kernel<FORMAT>, dim3((p.total + kThreads - 1u) / kThreads), dim3(kThreads), 0, ctx->stream, p);
    UR_HIP_TRY(hipGetLastError());
    return UR_OK;
}

bool chain_shape(uint32_t width, uint32_t height, uint32_t mips) { return width != 0u && height != 0u && width <= 65535u && height <= 65535u && mips != 0u && mips <= 255u; }

} // namespace
} // namespace ur

extern "C" {

uint64_t ur_texture_transcode_bytes(uint32_t width, uint32_t height, uint32_t mips)
{
    return ur::chain_shape(width, height, mips) ? 4u * ur_bc::chain_texels(width, height, mips) : 0u;
}

int ur_texture_transcode(ur_ctx* ctx, uint32_t source_format, const void* blocks, uint32_t width, uint32_t height, uint32_t mips, void* rgba8,
                         ur_texture2d* out_descriptor)
{
    using namespace ur;
    if (!ctx || !blocks || !rgba8) { set_error("ur_texture_transcode: null context, blocks or rgba8"); return UR_EINVAL; }
    if (!ur_bc::is_source(source_format)) { set_error("ur_texture_transcode: source format %u (71, 72, 74, 75, 77, 78, 80, 83, 98, 99)", source_format); return UR_EINVAL; }
    if (!chain_shape(width, height, mips)) { set_error("ur_texture_transcode: no chain: %u x %u, %u mips (sizes 1..65535, mips 1..255)", width, height, mips); return UR_EINVAL; }
    const uint32_t block_size = ur_bc::source_block_bytes(source_format);
    if (reinterpret_cast<uintptr_t>(blocks) % block_size != 0u) { set_error("ur_texture_transcode: blocks not aligned to the block size (%u bytes)", block_size); return UR_EINVAL; }
    if (reinterpret_cast<uintptr_t>(rgba8) % 4u != 0u) { set_error("ur_texture_transcode: rgba8 not 4-byte aligned"); return UR_EINVAL; }
    const size_t src_bytes = ur_bc::source_chain_bytes(source_format, width, height, mips), dst_bytes = (size_t)ur_texture_transcode_bytes(width, height, mips);
    if (overlaps(blocks, src_bytes, rgba8, dst_bytes)) { set_error("ur_texture_transcode: source and destination overlap"); return UR_EINVAL; }

    TranscodeParams p{};
    p.src = static_cast<const uint8_t*>(blocks);
    p.dst = static_cast<uint32_t*>(rgba8);
    p.width = width; p.height = height;
    const uint32_t sized = mips < 16u ? mips : 16u; // levels with a size of their own
    uint64_t items = 0u;
    for (uint32_t l = 0u; l < kLevels; ++l) {
        const uint32_t d = l < sized ? l : sized; // (the entries behind the chain's end are never selected: their start is `total`)
        p.src_block[l] = (uint32_t)ur_bc::chain_blocks(width, height, d);
        p.dst_texel[l] = ur_bc::chain_texels(width, height, d);
        p.start[l] = (uint32_t)items;
        if (l < sized) items += (uint64_t)ur_bc::level_size(height, l) * ur_bc::blocks_across(ur_bc::level_size(width, l));
    }
    items += mips - sized;
    for (uint32_t l = sized + (mips > 16u ? 1u : 0u); l < kLevels; ++l) p.start[l] = (uint32_t)items;
    p.total = (uint32_t)items; // (at most 65535 * 16384 * 4 / 3 + 255 < 2^31)

    int rc = UR_OK;
    switch (source_format) {
    case ur_bc::kBC1: case ur_bc::kBC1Srgb: rc = launch<ur_bc::kBC1>(ctx, p); break;
    case ur_bc::kBC2: case ur_bc::kBC2Srgb: rc = launch<ur_bc::kBC2>(ctx, p); break;
    case ur_bc::kBC3: case ur_bc::kBC3Srgb: rc = launch<ur_bc::kBC3>(ctx, p); break;
    case ur_bc::kBC4: rc = launch<ur_bc::kBC4>(ctx, p); break;
    case ur_bc::kBC5: rc = launch<ur_bc::kBC5>(ctx, p); break;
    default: rc = launch<ur_bc::kBC7>(ctx, p); break;
    }
    if (rc != UR_OK) return rc;
    if (out_descriptor) {
        out_descriptor->texels = reinterpret_cast<uint64_t>(rgba8);
        out_descriptor->width = (uint16_t)width; out_descriptor->height = (uint16_t)height;
        out_descriptor->mips = (uint8_t)mips;
        out_descriptor->format = (uint8_t)(ur_bc::source_is_srgb(source_format) ? UR_TEXTURE_R8G8B8A8_UNORM_SRGB : UR_TEXTURE_R8G8B8A8_UNORM);
        out_descriptor->reserved = 0u;
    }
    return UR_OK;
}

} // extern "C"
