// The kernel arguments of CullIndirectArgs (cull_kernels.h): the reference's constants and the call's buffers, the camera's draw
// ranges, the extra views, and the zeroing launch's.
#pragma once

#include "ur_internal.h"
#include "ur_device.h"

namespace {

struct CullParams {
    // CullingConstants, CullIndirectArgs.hlsl:1-11
    float4 FrustumPlanes[6];
    float ViewProjection[16];
    uint32_t ModelCount, HZBEnabled, HZBMipCount, HZBWidth, HZBHeight, DebugPrintEnabled;
    const float4* bounds;
    const float* hzb;
    uint8_t* args;
    uint32_t* stats;
    uint32_t* visible_idx;
    uint32_t* visible_count;
    uint32_t* block_counts;
    uint64_t* wave_masks;
    uint32_t index_base;
    uint32_t store_flavour;
    uint32_t record_valid; // store_flavour 4: wave_masks holds the visible bits this context's previous launch left in THIS command buffer
    uint32_t mip_offset[UR_MAX_HZB_MIPS];
    uint32_t mip_width[UR_MAX_HZB_MIPS];
    unsigned long long* timeline; // debug: {first entry, last exit} of this launch (ur_debug_timeline), else null
};
// the constants are copied over the head of CullParams as they come (cull_launch.h)
static_assert(sizeof(float4) * 6 + sizeof(float) * 16 + 6 * 4 == UR_CULL_CONSTANT_DWORDS * 4, "46 dwords");

// ur_draw_ranges on the device
struct DrawParams {
    const uint32_t* offsets; // [range_count + 1], offsets[0] = 0, non-decreasing, offsets[range_count] = ModelCount
    uint8_t* commands;
    uint32_t* counts;
    uint32_t range_count;
};

// ur_cull_view[] on the device. A view without ranges has D.range_count == 0; block_counts / wave_masks are its slice of the
// context's scratch (set when the view has a list or ranges and the call has more than one block)
struct ViewParams {
    float4 planes[UR_MAX_CULL_VIEWS][6];
    uint32_t* mask[UR_MAX_CULL_VIEWS];
    uint32_t* visible_idx[UR_MAX_CULL_VIEWS];
    uint32_t* visible_count[UR_MAX_CULL_VIEWS];
    DrawParams D[UR_MAX_CULL_VIEWS];
    uint32_t* block_counts[UR_MAX_CULL_VIEWS];
    uint64_t* wave_masks[UR_MAX_CULL_VIEWS];
    uint32_t count; // 1..UR_MAX_CULL_VIEWS
};

// The kernel arguments: CullParams alone without ranges (the layout the kernels always had), CullParams + DrawParams with them;
// + ViewParams with views
template <bool RANGES, bool VIEWS = false> struct CullArgs : CullParams { DrawParams D; ViewParams V; };
template <> struct CullArgs<false, true> : CullParams { ViewParams V; };
template <> struct CullArgs<true, false> : CullParams { DrawParams D; };
template <> struct CullArgs<false, false> : CullParams {};

// ModelCount == 0: every count (camera's and views') and every counts[r], one launch
struct ZeroArgs {
    uint32_t* count[1 + UR_MAX_CULL_VIEWS];
    uint32_t* counts[1 + UR_MAX_CULL_VIEWS];
    uint32_t range_count[1 + UR_MAX_CULL_VIEWS];
};

} // namespace
