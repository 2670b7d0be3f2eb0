// CullIndirectArgs with extra views (ur_cull_indirect_args_views): the launches of cull_kernel / compact_kernel with VIEWS (see
// cull_kernels.h). A translation unit of its own, so that the camera-only kernels in cull.hip compile exactly as they did without views.

#include "cull_kernels.h"

namespace ur {

namespace {

// The launches of a call with n > 256 (blocks >= 2): the cull, then the compaction when there is a list or there are ranges (with
// views: the camera's or any view's; one row per view behind the camera's)
template <bool RANGES, bool VIEWS>
int launch_blocks(ur_ctx* ctx, const CullArgs<RANGES, VIEWS>& P, uint32_t blocks, hipEvent_t stop)
{
    bool compact = RANGES || P.visible_idx != nullptr;
    uint32_t rows = 1;
    if constexpr (VIEWS) {
        for (uint32_t v = 0; v < P.V.count; ++v) compact = compact || P.V.wave_masks[v] != nullptr;
        rows = 1u + P.V.count;
    }
    const auto cull = cull_kernel<false, RANGES, VIEWS>;
    const auto compaction = compact_kernel<RANGES, VIEWS>;
    if (stop != nullptr && !compact) hipExtLaunchKernelGGL(cull, dim3(blocks), dim3(256), 0, ctx->stream, nullptr, stop, 0, P);
    else hipLaunchKernelGGL(cull, dim3(blocks), dim3(256), 0, ctx->stream, P);
    UR_HIP_TRY(hipGetLastError());
    if (compact) {
        const dim3 grid((blocks * 4u + 255u) / 256u, rows);
        if (stop != nullptr) hipExtLaunchKernelGGL(compaction, grid, dim3(256), 0, ctx->stream, nullptr, stop, 0, P, blocks);
        else hipLaunchKernelGGL(compaction, grid, dim3(256), 0, ctx->stream, P, blocks);
        UR_HIP_TRY(hipGetLastError());
    }
    return UR_OK;
}

// The single-block launch: cull_kernel<true, ...> carries the call's event
template <bool RANGES, bool VIEWS>
int launch_single(ur_ctx* ctx, const CullArgs<RANGES, VIEWS>& P, hipEvent_t stop)
{
    const auto single = cull_kernel<true, RANGES, VIEWS>;
    if (stop != nullptr) hipExtLaunchKernelGGL(single, dim3(1), dim3(256), 0, ctx->stream, nullptr, stop, 0, P);
    else hipLaunchKernelGGL(single, dim3(1), dim3(256), 0, ctx->stream, P);
    UR_HIP_TRY(hipGetLastError());
    return UR_OK;
}

} // namespace

int launch_cull_views(ur_ctx* ctx, const uint32_t* constants, const ur_float4* bounds, const float* hzb, const ur_mip_desc* mips,
                      void* indirect_args, uint32_t* stats2, uint32_t* visible_idx, uint32_t* visible_count, uint32_t index_base,
                      const ur_draw_ranges* draws, const ur_cull_view* views, uint32_t view_count)
{
    CullArgs<true, true> P{};
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
    P.V.count = view_count;
    for (uint32_t v = 0; v < view_count; ++v) {
        std::memcpy(P.V.planes[v], views[v].planes, sizeof(P.V.planes[v]));
        P.V.mask[v] = views[v].mask;
        P.V.visible_idx[v] = views[v].visible_idx;
        P.V.visible_count[v] = views[v].visible_count;
        if (const ur_draw_ranges* d = views[v].draws) P.V.D[v] = {d->offsets, static_cast<uint8_t*>(d->commands), d->counts, d->range_count};
    }
    CullArgs<false, true> PV{}; // (the same without the camera's ranges)
    static_cast<CullParams&>(PV) = P;
    PV.V = P.V;
    // ur_time_next_cull: the call's LAST launch carries the event on its dispatch (its completion stamp is somebody's start time).
    // (ur_cull_indirect_args_ex clears the context's copy behind this function on every path: a raw hipEvent_t must not stay in
    // the context for a later call.)
    hipEvent_t stop = ctx->time_cull_stop;
    const uint32_t n = P.ModelCount;
    if (n == 0) {
        ctx->cull_record_args = nullptr;
        bool zero = visible_count != nullptr || draws != nullptr;
        for (uint32_t v = 0; v < view_count; ++v) zero = zero || views[v].visible_count || views[v].draws;
        if (zero) { // one launch zeroes every count and every counts[r] (no mask word is written)
            ZeroArgs Z{};
            uint32_t most = draws ? draws->range_count : 0u;
            Z.count[0] = visible_count;
            if (draws) { Z.counts[0] = draws->counts; Z.range_count[0] = draws->range_count; }
            for (uint32_t v = 0; v < view_count; ++v) {
                Z.count[1 + v] = views[v].visible_count;
                if (views[v].draws) {
                    Z.counts[1 + v] = views[v].draws->counts;
                    Z.range_count[1 + v] = views[v].draws->range_count;
                    most = std::max(most, views[v].draws->range_count);
                }
            }
            const uint32_t grid = std::max(1u, (uint32_t)(((uint64_t)most + 255u) / 256u));
            if (stop != nullptr) hipExtLaunchKernelGGL(zero_views_kernel, dim3(grid), dim3(256), 0, ctx->stream, nullptr, stop, 0, Z);
            else hipLaunchKernelGGL(zero_views_kernel, dim3(grid), dim3(256), 0, ctx->stream, Z);
            UR_HIP_TRY(hipGetLastError());
            ctx->time_cull_carried = stop != nullptr;
        }
        return UR_OK;
    }
    const uint32_t blocks = (n + 255u) / 256u;
    if (blocks == 1) {
        ctx->cull_record_args = nullptr; // (one block keeps no masks)
        const int rc = draws ? launch_single(ctx, P, stop) : launch_single(ctx, PV, stop);
        if (rc != UR_OK) return rc;
        ctx->time_cull_carried = stop != nullptr;
        return UR_OK;
    }
    { // the masks and block counts: the compaction's input, flavour 4's record (the camera's are always written with views)
        if (n > ctx->ws_instances) {
            const int rc = ur_reserve(ctx, n); // (a new workspace forgets the record)
            if (rc != UR_OK) return rc;
        }
        // slice 0 is the camera's (and flavour 4's record); view v's is slice 1 + v
        const uint32_t stride = ctx->ws_instances / 256u;
        P.block_counts = PV.block_counts = ctx->block_counts;
        P.wave_masks = PV.wave_masks = ctx->wave_masks;
        for (uint32_t v = 0; v < view_count; ++v) { // (a view with a list or ranges)
            if (!views[v].visible_idx && !views[v].draws) continue;
            P.V.block_counts[v] = PV.V.block_counts[v] = ctx->block_counts + (size_t)(1u + v) * stride;
            P.V.wave_masks[v] = PV.V.wave_masks[v] = ctx->wave_masks + (size_t)(1u + v) * stride * 4u;
        }
    }
    // UR_OPT_CULL_STORE = 4: the wave masks ARE the record of what this launch leaves in the command buffer; they describe the buffer the
    // next launch meets if that launch is on the same buffer with the same count (and the caller keeps the promise of the option)
    const uint32_t record_valid = (P.store_flavour == 4u && ctx->cull_record_args == indirect_args && ctx->cull_record_n == n) ? 1u : 0u;
    P.record_valid = PV.record_valid = record_valid;
    ctx->cull_record_args = P.store_flavour == 4u ? indirect_args : nullptr;
    ctx->cull_record_n = n;
    const int rc = draws ? launch_blocks(ctx, P, blocks, stop) : launch_blocks(ctx, PV, blocks, stop);
    if (rc != UR_OK) return rc;
    ctx->time_cull_carried = stop != nullptr;
    return UR_OK;
}

} // namespace ur
