// The raster of ShadowMap, DepthPrepass and GBuffer's opaque draws for gfx950: the launches of the raster kernels (csrc/raster_kernels.h)
// under the Shadow, Depth and Vis policies (csrc/raster_policies.h), the checks of an ur_raster_draws (ur_internal.h) and
// ur_shadow_map / ur_depth_prepass / ur_raster_reserve. GBuffer's alpha-masked draws are csrc/raster_mask.hip, the ObjectId pick
// csrc/raster_pick.hip. Built with -ffp-contract=off.

#include "raster_kernels.h"

// ---- what the direct calls and the frame's setters (frame/FrameApi.cpp) share (ur_checks.h); `who` goes into the error text ----
int ur::check_raster_draws(const char* who, const ur_raster_draws& draws, const void* target, const char* target_name, const void* stats)
{
    if (!target) { set_error("%s: null %s", who, target_name); return UR_EINVAL; }
    const bool list = draws.visible_idx != nullptr || draws.visible_count != nullptr;
    if (list && (!draws.visible_idx || !draws.visible_count)) { set_error("%s: a list needs visible_idx and visible_count", who); return UR_EINVAL; }
    if (list && draws.ranges) { set_error("%s: a list and ranges at once", who); return UR_EINVAL; }
    const ur_draw_ranges* rg = draws.ranges;
    if (rg && (!rg->offsets || !rg->commands || !rg->counts || rg->range_count == 0u)) { set_error("%s: a null member of ranges / no range", who); return UR_EINVAL; }
    const void* commands = raster_commands(draws);
    if (!commands && draws.command_count != 0u) { set_error("%s: null commands", who); return UR_EINVAL; }
    if (!aligned(commands, 16) || !aligned(target, 4) || !aligned(stats, 4) || !aligned(draws.visible_idx, 4) || !aligned(draws.visible_count, 4) ||
        (rg && (!aligned(rg->offsets, 4) || !aligned(rg->counts, 4)))) {
        set_error("%s: a misaligned buffer (commands 16 bytes, the others 4)", who);
        return UR_EINVAL;
    }
    return UR_OK;
}

int ur::check_raster_call(const char* who, const ur_ctx* ctx, const float* m0, const float* m1, const ur_raster_draws* draws, const void* target, const char* target_name,
                          uint32_t w, uint32_t h, const void* stats)
{
    if (!ctx || !m0 || !m1 || !draws) { set_error("%s: null context, matrix or draws", who); return UR_EINVAL; }
    if (w == 0u || h == 0u || w > UR_RASTER_MAX_TARGET || h > UR_RASTER_MAX_TARGET) { set_error("%s: a %u x %u target (1..%u)", who, w, h, UR_RASTER_MAX_TARGET); return UR_EINVAL; }
    return check_raster_draws(who, *draws, target, target_name, stats);
}

int ur::launch_visibility_raster(ur_ctx* ctx, const float* view, const float* projection, const ur_raster_draws* draws, const float* depth, uint32_t* keys, uint32_t w,
                                 uint32_t h, uint32_t row0, uint32_t rows, uint32_t key_bits, bool d24, uint32_t* stats)
{
    const VisArgs vis{depth, row0, rows, key_bits};
    if (d24) return launch_raster<VisPolicy<true>>(ctx, view, projection, draws, keys, w * rows, w, h, 0.0f, stats, &vis);
    return launch_raster<VisPolicy<false>>(ctx, view, projection, draws, keys, w * rows, w, h, 0.0f, stats, &vis);
}

extern "C" {

int ur_raster_reserve(ur_ctx* ctx, uint32_t max_large_work_items)
{
    if (!ctx) { ur::set_error("ur_raster_reserve: null context"); return UR_EINVAL; }
    if (max_large_work_items == ctx->raster_queue_cap) return UR_OK;
    UR_HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (ctx->raster_queue) (void)hipFree(ctx->raster_queue);
    ctx->raster_queue = nullptr;
    ctx->raster_queue_cap = 0;
    if (max_large_work_items == 0u) return UR_OK;
    const size_t bytes = ((size_t)kQueueHeaderDwords + (size_t)max_large_work_items * kKeyedEntryDwords) * sizeof(uint32_t);
    if (hipMalloc(&ctx->raster_queue, bytes) != hipSuccess) {
        ctx->raster_queue = nullptr;
        ur::set_error("ur_raster_reserve: allocation of %u large work items failed", max_large_work_items);
        return UR_ENOMEM;
    }
    ctx->raster_queue_cap = max_large_work_items;
    return UR_OK;
}

int ur_shadow_map(ur_ctx* ctx, const float* lvp, const ur_raster_draws* draws, float* shadow_map, uint32_t w, uint32_t h, uint32_t* stats4)
{
    const int rc = ur::check_raster_call("ur_shadow_map", ctx, lvp, lvp, draws, shadow_map, "shadow_map", w, h, stats4);
    if (rc != UR_OK) return rc;
    if (!(lvp[3] == 0.0f && lvp[7] == 0.0f && lvp[11] == 0.0f && lvp[15] == 1.0f)) {
        ur::set_error("ur_shadow_map: the light's fourth column is (%g, %g, %g, %g), not (0, 0, 0, 1): only orthographic lights are rasterised", lvp[3], lvp[7], lvp[11], lvp[15]);
        return UR_EUNSUPPORTED;
    }
    return launch_raster<ShadowPolicy>(ctx, lvp, nullptr, draws, reinterpret_cast<uint32_t*>(shadow_map), w * h, w, h, 1.0f, stats4, nullptr);
}

int ur_depth_prepass(ur_ctx* ctx, const float* view, const float* projection, const ur_raster_draws* draws, float* depth, uint32_t w, uint32_t h, uint32_t flags,
                     uint32_t* stats6)
{
    int rc = ur::check_raster_call("ur_depth_prepass", ctx, view, projection, draws, depth, "depth", w, h, stats6);
    if (rc == UR_OK) rc = ur::check_depth_flags("ur_depth_prepass", flags);
    if (rc != UR_OK) return rc;
    if (flags & UR_DEPTH_QUANTIZE_D24) return launch_raster<DepthPolicy<true>>(ctx, view, projection, draws, reinterpret_cast<uint32_t*>(depth), w * h, w, h, 0.0f, stats6, nullptr);
    return launch_raster<DepthPolicy<false>>(ctx, view, projection, draws, reinterpret_cast<uint32_t*>(depth), w * h, w, h, 0.0f, stats6, nullptr);
}

} // extern "C"
