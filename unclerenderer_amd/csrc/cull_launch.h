// The one host launch path of the CullIndirectArgs kernels (cull_kernels.h), shared by cull.hip and cull_views.hip: fill the kernel
// arguments, plan the call (cull_plan.cpp: every decision - the launches and their grids, the workspace and its slices, the record of
// UR_OPT_CULL_STORE = 4, the dispatch that carries ur_time_next_cull's event), bind the plan to buffers and kernels.
#pragma once

#include "cull_kernels.h"
#include "cull_plan.h"

#include <hip/hip_ext.h>

#include <algorithm>
#include <cstring>

namespace {

// One 256-thread launch on the context's stream; with `stop` (ur_time_next_cull) its dispatch carries the event
template <class K, class... Args>
int launch_stop(ur_ctx* ctx, hipEvent_t stop, K kernel, dim3 grid, const Args&... args)
{
    if (stop != nullptr) hipExtLaunchKernelGGL(kernel, grid, dim3(256), 0, ctx->stream, nullptr, stop, 0, args...);
    else hipLaunchKernelGGL(kernel, grid, dim3(256), 0, ctx->stream, args...);
    UR_HIP_TRY(hipGetLastError());
    return UR_OK;
}

DrawParams draw_params(const ur_draw_ranges& d) { return {d.offsets, static_cast<uint8_t*>(d.commands), d.counts, d.range_count}; }

// The launches of one cull call after the HZB tail is flushed: the camera alone (VIEWS = false, cull.hip) or with view_count >= 1
// extra views (cull_views.hip). Each translation unit instantiates it once, so each module holds its own set of kernels only.
template <bool VIEWS>
int cull_launches(ur_ctx* ctx, const uint32_t* constants, const ur_float4* bounds, const float* hzb, const ur_mip_desc* mips,
                  void* indirect_args, uint32_t* stats2, uint32_t* visible_idx, uint32_t* visible_count, uint32_t index_base,
                  const ur_draw_ranges* draws, const ur_cull_view* views, uint32_t view_count)
{
    if constexpr (!VIEWS) view_count = 0;
    // ---- the arguments: P with the camera's ranges, Q the same without them (filled from P in front of the launches), Z the zeroing launch's
    CullArgs<true, VIEWS> P{};
    CullArgs<false, VIEWS> Q{};
    ZeroArgs Z{};
    std::memcpy(static_cast<CullParams*>(&P), constants, UR_CULL_CONSTANT_DWORDS * 4);
    P.bounds = reinterpret_cast<const float4*>(bounds);
    P.hzb = hzb;
    P.args = static_cast<uint8_t*>(indirect_args);
    P.stats = stats2;
    P.visible_idx = visible_idx;
    P.visible_count = visible_count;
    P.index_base = index_base;
    P.store_flavour = (uint32_t)ctx->opt.cull_store; // UR_OPT_CULL_STORE
    P.timeline = P.ModelCount != 0 ? ur::next_timeline_pair(ctx) : nullptr; // (the compaction launch of a large cull is not stamped)
    if (P.HZBEnabled != 0) {
        for (uint32_t m = 0; m < P.HZBMipCount && m < UR_MAX_HZB_MIPS; ++m) {
            P.mip_offset[m] = mips[m].offset;
            P.mip_width[m] = mips[m].width;
        }
    }
    const uint32_t n = P.ModelCount;
    ur::CullPlanInput in{};
    in.n = n;
    in.camera_list = visible_idx != nullptr; // (the entry point has checked that the list and its count go together)
    in.camera_ranges = draws != nullptr;
    in.view_count = view_count;
    Z.count[0] = visible_count;
    if (draws) {
        P.D = draw_params(*draws);
        Z.counts[0] = draws->counts;
        Z.range_count[0] = in.most_ranges = draws->range_count;
    }
    if constexpr (VIEWS) {
        P.V.count = view_count;
        for (uint32_t v = 0; v < view_count; ++v) {
            std::memcpy(P.V.planes[v], views[v].planes, sizeof(P.V.planes[v]));
            P.V.mask[v] = views[v].mask;
            P.V.visible_idx[v] = views[v].visible_idx;
            P.V.visible_count[v] = views[v].visible_count;
            Z.count[1 + v] = views[v].visible_count;
            // a view with a list or ranges (compacted, with a scratch slice of its own, above one block)
            in.view_compacted[v] = views[v].visible_idx != nullptr || views[v].draws != nullptr;
            if (views[v].draws) {
                P.V.D[v] = draw_params(*views[v].draws);
                Z.counts[1 + v] = views[v].draws->counts;
                Z.range_count[1 + v] = views[v].draws->range_count;
                in.most_ranges = std::max(in.most_ranges, views[v].draws->range_count);
            }
        }
    }
    // ---- the plan. UR_OPT_CULL_STORE = 4: the wave masks ARE the record of what a multi-block launch leaves in the command buffer; they
    // describe the buffer the next launch meets if that launch is on the same buffer with the same count (and the caller keeps the promise
    // of the option). The record is forgotten here and kept again only once every launch of this call has gone out.
    in.store_flavour = P.store_flavour;
    in.record_same_buffer = ctx->cull_record_args == indirect_args;
    in.record_same_count = ctx->cull_record_n == n;
    in.ws_instances = ctx->ws_instances;
    in.stop_armed = ctx->time_cull_stop != nullptr;
    const ur::CullPlan plan = ur::plan_cull(in);
    ctx->cull_record_args = nullptr;
    // ur_time_next_cull: the call's LAST launch carries the event on its dispatch (its completion stamp is somebody's start time).
    // (The entry point clears the context's copy behind this function on every path: a raw hipEvent_t must not stay in the context.)
    auto stop_on = [&](ur::CullPlan::StopOn step) { return plan.stop_on == step ? ctx->time_cull_stop : nullptr; };

    // ---- the plan's steps, bound to buffers and kernels
    int rc = UR_OK;
    switch (plan.kind) {
    case ur::CullPlan::nothing: return UR_OK;
    case ur::CullPlan::zero: // one launch zeroes every count and every counts[r] (no mask word is written)
        rc = launch_stop(ctx, stop_on(ur::CullPlan::only), zero_views_kernel, dim3(plan.zero_grid), Z);
        break;
    case ur::CullPlan::single_block:
        static_cast<CullParams&>(Q) = P;
        if constexpr (VIEWS) Q.V = P.V;
        rc = plan.ranges ? launch_stop(ctx, stop_on(ur::CullPlan::only), cull_kernel<true, true, VIEWS>, dim3(1), P)
                         : launch_stop(ctx, stop_on(ur::CullPlan::only), cull_kernel<true, false, VIEWS>, dim3(1), Q);
        break;
    case ur::CullPlan::multi_block:
        if (plan.reserve_to != 0) {
            rc = ur_reserve(ctx, plan.reserve_to);
            if (rc != UR_OK) return rc;
            if (ctx->ws_instances != plan.ws_instances) { // (the plan's slices lie where ur_reserve's rounding puts them: the two must agree)
                ur::set_error("ur_cull_indirect_args: ur_reserve left a workspace of %u instances, the plan expects %u", ctx->ws_instances, plan.ws_instances);
                return UR_EINVAL;
            }
        }
        if (plan.needs_workspace) { // slice 0 is the camera's (and flavour 4's record); view v's is slice plan.view_slice[v] = 1 + v
            P.block_counts = ctx->block_counts;
            P.wave_masks = ctx->wave_masks;
            if constexpr (VIEWS) {
                for (uint32_t v = 0; v < view_count; ++v) {
                    if (plan.view_slice[v] < 0) continue;
                    P.V.block_counts[v] = ctx->block_counts + (size_t)plan.view_slice[v] * plan.stride;
                    P.V.wave_masks[v] = ctx->wave_masks + (size_t)plan.view_slice[v] * plan.stride * 4u;
                }
            }
        }
        P.record_valid = plan.record_valid ? 1u : 0u;
        static_cast<CullParams&>(Q) = P;
        if constexpr (VIEWS) Q.V = P.V;
        // the cull, then the compaction when there is a list or there are ranges: one row of workgroups for the camera, one per view
        rc = plan.ranges ? launch_stop(ctx, stop_on(ur::CullPlan::cull), cull_kernel<false, true, VIEWS>, dim3(plan.blocks), P)
                         : launch_stop(ctx, stop_on(ur::CullPlan::cull), cull_kernel<false, false, VIEWS>, dim3(plan.blocks), Q);
        if (rc == UR_OK && plan.compact) {
            const dim3 grid(plan.compact_grid_x, plan.compact_grid_y);
            rc = plan.ranges ? launch_stop(ctx, stop_on(ur::CullPlan::compaction), compact_kernel<true, VIEWS>, grid, P, plan.blocks)
                             : launch_stop(ctx, stop_on(ur::CullPlan::compaction), compact_kernel<false, VIEWS>, grid, Q, plan.blocks);
        }
        break;
    }
    if (rc != UR_OK) return rc;
    if (plan.keep_record) {
        ctx->cull_record_args = indirect_args;
        ctx->cull_record_n = n;
    }
    ctx->time_cull_carried = plan.carried();
    return UR_OK;
}

} // namespace
