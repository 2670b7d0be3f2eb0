// CullIndirectArgs for gfx950 — frustum + HZB occlusion cull of instance AABBs, plus the visible-list compaction the
// reference does not have.
//
// Reference: Shaders/CullIndirectArgs.hlsl:24-167 ([numthreads(64,1,1)], one thread per instance, writes the
// InstanceCount word at byte 44 of each 64-byte FIndirectDrawCommand), dispatched by FRenderer::DispatchGpuCulling
// (Source/Render/Renderer.cpp:394-472). The arithmetic below follows the HLSL statement by statement and this file is
// built with -ffp-contract=off and IEEE division so every intermediate equals the oracle's; floor(log2(x)) is taken from
// the IEEE exponent.
//
// MI355X shape: 256-thread workgroups (4 x wave64). The workgroup's 256 AABBs (8 KB) are staged through LDS with
// fully-coalesced 16-byte loads, then each lane reads its own min/max pair. Visibility is a wave ballot: lane 0 keeps
// the 64-bit mask, popcounts give per-wave and per-workgroup counts. Compaction is deterministic (ascending index, no
// atomic append): pass 1 stores per-wave masks and per-workgroup counts, pass 2 (one thread per mask) takes the exclusive
// prefix of the counts and writes out the set bits of its mask. Up to 256 instances (Sponza 25, pica_pica 170) both passes
// run inside one launch.
//
// Draw ranges (ur_cull_indirect_args_draws): the same two passes also place every visible command of range r, whole, at command
// slots offsets[r], offsets[r] + 1, ... of a second buffer and write counts[r], for ExecuteIndirect / vkCmdDrawIndexedIndirectCount
// with a count buffer. The work is the RANGES template parameter: the instantiations without it are the kernels as they were.
//
// Extra views (ur_cull_indirect_args_views): up to UR_MAX_CULL_VIEWS more frustums - the DepthPrepass's camera frustum, a light's
// view, cascades - tested with the reference's CPU test (RendererUtils IsAabbInCameraFrustum, no HZB) on the AABBs the launch has
// already staged in LDS. Each view writes its own bitmask, list and draw ranges; the lists and ranges go through the same compaction
// (one more launch row per view, its masks in its own slice of the context's scratch). The VIEWS template parameter: the
// instantiations without it are, again, the kernels as they were.
//
// The kernels are in cull_kernels.h (with cull_params.h, cull_tests.h, cull_compact.h), their launch path (cull_launches) in cull_launch.h,
// its decisions in cull_plan.cpp. This file instantiates the camera-only kernels, cull_views.hip those with views: each module holds one
// set, so the camera-only kernels compile exactly as they did before the views existed.

#include "cull_kernels.h"
#include "cull_launch.h"

namespace ur {

int launch_cull(ur_ctx* ctx, const uint32_t* constants, const ur_float4* bounds, const float* hzb, const ur_mip_desc* mips,
                void* indirect_args, uint32_t* stats2, uint32_t* visible_idx, uint32_t* visible_count, uint32_t index_base,
                const ur_draw_ranges* draws, const ur_cull_view* views, uint32_t view_count)
{
    const int rc = flush_hzb_tail(ctx); // the cull reads the whole chain
    if (rc != UR_OK) return rc;
    if (views != nullptr && view_count != 0) return launch_cull_views(ctx, constants, bounds, hzb, mips, indirect_args, stats2, visible_idx, visible_count, index_base, draws, views, view_count);
    return cull_launches<false>(ctx, constants, bounds, hzb, mips, indirect_args, stats2, visible_idx, visible_count, index_base, draws, nullptr, 0);
}

} // namespace ur
