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
// The kernels are in cull_kernels.h. This file launches the camera-only instantiations, cull_views.hip those with views: each module
// holds one set, so the camera-only kernels compile exactly as they did before the views existed.

#include "cull_kernels.h"

namespace ur {

namespace {

// The launches of a call with n > 256 (blocks >= 2): the cull, then the compaction when there is a list or there are ranges
template <bool RANGES>
int launch_blocks(ur_ctx* ctx, const CullArgs<RANGES>& P, uint32_t blocks, hipEvent_t stop)
{
    const bool compact = RANGES || P.visible_idx != nullptr;
    const auto cull = cull_kernel<false, RANGES>;
    const auto compaction = compact_kernel<RANGES>;
    if (stop != nullptr && !compact) hipExtLaunchKernelGGL(cull, dim3(blocks), dim3(256), 0, ctx->stream, nullptr, stop, 0, P);
    else hipLaunchKernelGGL(cull, dim3(blocks), dim3(256), 0, ctx->stream, P);
    UR_HIP_TRY(hipGetLastError());
    if (compact) {
        if (stop != nullptr) hipExtLaunchKernelGGL(compaction, dim3((blocks * 4u + 255u) / 256u), dim3(256), 0, ctx->stream, nullptr, stop, 0, P, blocks);
        else hipLaunchKernelGGL(compaction, dim3((blocks * 4u + 255u) / 256u), dim3(256), 0, ctx->stream, P, blocks);
        UR_HIP_TRY(hipGetLastError());
    }
    return UR_OK;
}

} // namespace

int launch_cull(ur_ctx* ctx, const uint32_t* constants, const ur_float4* bounds, const float* hzb, const ur_mip_desc* mips,
                void* indirect_args, uint32_t* stats2, uint32_t* visible_idx, uint32_t* visible_count, uint32_t index_base,
                const ur_draw_ranges* draws, const ur_cull_view* views, uint32_t view_count)
{
    {
        const int rc = flush_hzb_tail(ctx); // the cull reads the whole chain
        if (rc != UR_OK) return rc;
    }
    if (views != nullptr && view_count != 0) return launch_cull_views(ctx, constants, bounds, hzb, mips, indirect_args, stats2, visible_idx, visible_count, index_base, draws, views, view_count);
    CullArgs<true> P{};
    static_assert(sizeof(float4) * 6 + sizeof(float) * 16 + 6 * 4 == UR_CULL_CONSTANT_DWORDS * 4, "46 dwords");
    std::memcpy(static_cast<CullParams*>(&P), constants, UR_CULL_CONSTANT_DWORDS * 4);
    P.bounds = reinterpret_cast<const float4*>(bounds);
    P.hzb = hzb;
    P.args = static_cast<uint8_t*>(indirect_args);
    P.stats = stats2;
    P.visible_idx = visible_idx;
    P.visible_count = visible_count;
    P.index_base = index_base;
    P.store_flavour = (uint32_t)ctx->opt.cull_store; // UR_OPT_CULL_STORE
    P.timeline = P.ModelCount != 0 ? next_timeline_pair(ctx) : nullptr; // (the compaction launch of a large cull is not stamped)
    if (P.HZBEnabled != 0) {
        for (uint32_t m = 0; m < P.HZBMipCount && m < UR_MAX_HZB_MIPS; ++m) {
            P.mip_offset[m] = mips[m].offset;
            P.mip_width[m] = mips[m].width;
        }
    }
    if (draws) P.D = {draws->offsets, static_cast<uint8_t*>(draws->commands), draws->counts, draws->range_count};
    CullArgs<false> Q{};
    static_cast<CullParams&>(Q) = P; // (the same parameters without the ranges)
    // ur_time_next_cull: the call's LAST launch carries the event on its dispatch (its completion stamp is somebody's start time).
    // (ur_cull_indirect_args_ex clears the context's copy behind this function on every path: a raw hipEvent_t must not stay in
    // the context for a later call.)
    hipEvent_t stop = ctx->time_cull_stop;
    const uint32_t n = P.ModelCount;
    if (n == 0) {
        ctx->cull_record_args = nullptr;
        if (draws) { // one launch zeroes the counts (and the list's count)
            const uint32_t grid = (uint32_t)(((uint64_t)draws->range_count + 255u) / 256u);
            if (stop != nullptr) hipExtLaunchKernelGGL(zero_counts_kernel, dim3(grid), dim3(256), 0, ctx->stream, nullptr, stop, 0, visible_count, draws->counts, draws->range_count);
            else hipLaunchKernelGGL(zero_counts_kernel, dim3(grid), dim3(256), 0, ctx->stream, visible_count, draws->counts, draws->range_count);
            UR_HIP_TRY(hipGetLastError());
            ctx->time_cull_carried = stop != nullptr;
        } else if (visible_count) {
            if (stop != nullptr) hipExtLaunchKernelGGL(zero_count_kernel, dim3(1), dim3(1), 0, ctx->stream, nullptr, stop, 0, visible_count);
            else hipLaunchKernelGGL(zero_count_kernel, dim3(1), dim3(1), 0, ctx->stream, visible_count);
            UR_HIP_TRY(hipGetLastError());
            ctx->time_cull_carried = stop != nullptr;
        }
        return UR_OK;
    }
    const uint32_t blocks = (n + 255u) / 256u;
    if (blocks == 1) {
        ctx->cull_record_args = nullptr; // (one block keeps no masks)
        const auto single = cull_kernel<true, false>;
        const auto single_draws = cull_kernel<true, true>;
        if (draws) {
            if (stop != nullptr) hipExtLaunchKernelGGL(single_draws, dim3(1), dim3(256), 0, ctx->stream, nullptr, stop, 0, P);
            else hipLaunchKernelGGL(single_draws, dim3(1), dim3(256), 0, ctx->stream, P);
        } else {
            if (stop != nullptr) hipExtLaunchKernelGGL(single, dim3(1), dim3(256), 0, ctx->stream, nullptr, stop, 0, Q);
            else hipLaunchKernelGGL(single, dim3(1), dim3(256), 0, ctx->stream, Q);
        }
        UR_HIP_TRY(hipGetLastError());
        ctx->time_cull_carried = stop != nullptr;
        return UR_OK;
    }
    if (visible_idx || draws || P.store_flavour == 4u) { // the masks and block counts: the compaction's input, flavour 4's record
        if (n > ctx->ws_instances) {
            const int rc = ur_reserve(ctx, n); // (a new workspace forgets the record)
            if (rc != UR_OK) return rc;
        }
        P.block_counts = Q.block_counts = ctx->block_counts;
        P.wave_masks = Q.wave_masks = ctx->wave_masks;
    }
    // UR_OPT_CULL_STORE = 4: the wave masks ARE the record of what this launch leaves in the command buffer; they describe the buffer the
    // next launch meets if that launch is on the same buffer with the same count (and the caller keeps the promise of the option)
    P.record_valid = Q.record_valid = (P.store_flavour == 4u && ctx->cull_record_args == indirect_args && ctx->cull_record_n == n) ? 1u : 0u;
    ctx->cull_record_args = P.store_flavour == 4u ? indirect_args : nullptr;
    ctx->cull_record_n = n;
    const int rc = draws ? launch_blocks<true>(ctx, P, blocks, stop) : launch_blocks<false>(ctx, Q, blocks, stop);
    if (rc != UR_OK) return rc;
    ctx->time_cull_carried = stop != nullptr;
    return UR_OK;
}

} // namespace ur
