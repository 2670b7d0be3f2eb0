// CullIndirectArgs' entry points (include/ur_hotpath.h): every check of the constants, draw ranges and extra views, with its error
// text; the launches are cull.hip's and cull_views.hip's. Host code only.

#include "ur_internal.h"

using ur::set_error;

// What is wrong with one set of draw ranges, the camera's or a view's, against indirect_args. n = ModelCount, or ~0 when the commands
// are not known yet (the frame's copy of the views): the overlap and alignment checks then wait for the call.
enum class DrawsFault { none, member, overlap, alignment };
static DrawsFault check_draws(const ur_draw_ranges& d, uint32_t n, const void* indirect_args)
{
    if (!d.offsets || !d.commands || !d.counts || d.range_count == 0) return DrawsFault::member;
    if (n == ~0u || n == 0) return DrawsFault::none;
    const size_t bytes = (size_t)n * UR_INDIRECT_COMMAND_STRIDE;
    if (ur::overlaps(d.commands, bytes, indirect_args, bytes)) return DrawsFault::overlap;
    if (((reinterpret_cast<uintptr_t>(d.commands) | reinterpret_cast<uintptr_t>(indirect_args)) & 15u) != 0) return DrawsFault::alignment;
    return DrawsFault::none;
}

static int cull_checked(ur_ctx* ctx, const uint32_t* constants, const ur_float4* bounds, const float* hzb_base,
                        const ur_mip_desc* mips, void* indirect_args, uint32_t* stats2, uint32_t* visible_idx,
                        uint32_t* visible_count, uint32_t index_base, const ur_draw_ranges* draws,
                        const ur_cull_view* views, uint32_t view_count)
{
    if (!ctx || !constants) { set_error("ur_cull_indirect_args: null ctx/constants"); return UR_EINVAL; }
    const uint32_t n = constants[40], hzb_on = constants[41], mipc = constants[42];
    if ((visible_idx == nullptr) != (visible_count == nullptr)) { set_error("ur_cull_indirect_args: visible_idx and visible_count go together"); return UR_EINVAL; }
    if (n != 0 && (!bounds || !indirect_args)) { set_error("ur_cull_indirect_args: null bounds/indirect_args"); return UR_EINVAL; }
    if (n != 0 && hzb_on != 0 && constants[43] != 0 && constants[44] != 0 && mipc != 0) {
        if (!hzb_base || !mips || mipc > UR_MAX_HZB_MIPS) { set_error("ur_cull_indirect_args: HZB enabled but hzb/mips missing"); return UR_EINVAL; }
        if (mips[0].width != constants[43] || mips[0].height != constants[44]) { set_error("ur_cull_indirect_args: HZBWidth/Height do not match mips[0]"); return UR_EINVAL; }
        // the kernel indexes hzb + mips[level].offset with pitch mips[level].width for every level up to HZBMipCount - 1
        if (!ur::valid_hzb_chain_below_mip0(mips, mipc)) { set_error("ur_cull_indirect_args: mips[1..%u] do not halve from mips[0] / overlap", mipc - 1); return UR_EINVAL; }
    }
    switch (draws ? check_draws(*draws, n, indirect_args) : DrawsFault::none) {
    case DrawsFault::none: break;
    case DrawsFault::member: set_error("ur_cull_indirect_args_draws: null member / no range"); return UR_EINVAL;
    case DrawsFault::overlap: set_error("ur_cull_indirect_args_draws: commands overlap indirect_args"); return UR_EINVAL;
    case DrawsFault::alignment: set_error("ur_cull_indirect_args_draws: commands / indirect_args not 16-byte aligned"); return UR_EINVAL;
    }
    const int trc = ur::check_hzb_timeout(ctx, "ur_cull_indirect_args");
    if (trc != UR_OK) return trc;
    return ur::launch_cull(ctx, constants, bounds, hzb_base, mips, indirect_args, stats2, visible_idx, visible_count, index_base, draws,
                           views, view_count);
}

// The arguments of the views that need no device (ur_cull_indirect_args_views, ur_frame_set_cull_views). n = ModelCount, or ~0 when
// the commands are not known yet (the frame's copy): the overlap and alignment checks of the command buffers then wait for the call.
static int check_views(const char* who, const ur_cull_view* views, uint32_t view_count, uint32_t n, const void* indirect_args,
                       const ur_draw_ranges* draws)
{
    if (!views || view_count == 0) return UR_OK;
    if (view_count > UR_MAX_CULL_VIEWS) { set_error("%s: %u views (at most %u)", who, view_count, (uint32_t)UR_MAX_CULL_VIEWS); return UR_EINVAL; }
    const bool known = n != ~0u;
    const size_t bytes = known ? (size_t)n * UR_INDIRECT_COMMAND_STRIDE : 0u; // of a command buffer; 0: it cannot overlap another
    auto overlap = [&](const void* x, const void* y) { return ur::overlaps(x, bytes, y, bytes); };
    for (uint32_t v = 0; v < view_count; ++v) {
        const ur_cull_view& V = views[v];
        if (!V.mask && !V.visible_idx && !V.visible_count && !V.draws) { set_error("%s: view %u asks for nothing (no mask, list or ranges)", who, v); return UR_EINVAL; }
        if ((V.visible_idx == nullptr) != (V.visible_count == nullptr)) { set_error("%s: view %u: visible_idx and visible_count go together", who, v); return UR_EINVAL; }
        if (((reinterpret_cast<uintptr_t>(V.mask) | reinterpret_cast<uintptr_t>(V.visible_idx) | reinterpret_cast<uintptr_t>(V.visible_count)) & 3u) != 0) {
            set_error("%s: view %u: mask / visible_idx / visible_count not 4-byte aligned", who, v);
            return UR_EINVAL;
        }
        const ur_draw_ranges* d = V.draws;
        if (!d) continue;
        switch (check_draws(*d, n, indirect_args)) {
        case DrawsFault::none: break;
        case DrawsFault::member: set_error("%s: view %u: null member of draws / no range", who, v); return UR_EINVAL;
        case DrawsFault::overlap: set_error("%s: view %u: commands overlap indirect_args", who, v); return UR_EINVAL;
        case DrawsFault::alignment: set_error("%s: view %u: commands / indirect_args not 16-byte aligned", who, v); return UR_EINVAL;
        }
        if (draws && draws->commands && overlap(d->commands, draws->commands)) { set_error("%s: view %u: commands overlap the camera's commands", who, v); return UR_EINVAL; }
        for (uint32_t u = 0; u < v; ++u)
            if (views[u].draws && views[u].draws->commands && overlap(d->commands, views[u].draws->commands)) {
                set_error("%s: view %u: commands overlap view %u's", who, v, u);
                return UR_EINVAL;
            }
    }
    return UR_OK;
}

// Every ur_cull_indirect_args* entry point (views == NULL or view_count == 0: the camera alone). ur_time_next_cull's event is one-shot:
// cleared here whatever the call did, and ur_time_cull_carried reports whether a dispatch of THIS call took it.
static int cull_call(ur_ctx* ctx, const uint32_t* constants, const ur_float4* bounds, const float* hzb_base, const ur_mip_desc* mips,
                     void* indirect_args, uint32_t* stats2, uint32_t* visible_idx, uint32_t* visible_count, uint32_t index_base,
                     const ur_draw_ranges* draws, const ur_cull_view* views, uint32_t view_count)
{
    if (ctx) ctx->time_cull_carried = false;
    int rc = check_views("ur_cull_indirect_args_views", views, view_count, constants ? constants[40] : 0u, indirect_args, draws);
    if (rc == UR_OK) rc = cull_checked(ctx, constants, bounds, hzb_base, mips, indirect_args, stats2, visible_idx, visible_count, index_base, draws,
                                       views, views ? view_count : 0u);
    if (ctx) ctx->time_cull_stop = nullptr;
    return rc;
}

extern "C" {

int ur_cull_indirect_args(ur_ctx* ctx, const uint32_t* constants, const ur_float4* bounds, const float* hzb_base,
                          const ur_mip_desc* mips, void* indirect_args, uint32_t* stats2, uint32_t* visible_idx,
                          uint32_t* visible_count)
{
    return cull_call(ctx, constants, bounds, hzb_base, mips, indirect_args, stats2, visible_idx, visible_count, 0, nullptr, nullptr, 0);
}

int ur_cull_indirect_args_ex(ur_ctx* ctx, const uint32_t* constants, const ur_float4* bounds, const float* hzb_base,
                             const ur_mip_desc* mips, void* indirect_args, uint32_t* stats2, uint32_t* visible_idx,
                             uint32_t* visible_count, uint32_t index_base)
{
    return cull_call(ctx, constants, bounds, hzb_base, mips, indirect_args, stats2, visible_idx, visible_count, index_base, nullptr, nullptr, 0);
}

int ur_cull_indirect_args_draws(ur_ctx* ctx, const uint32_t* constants, const ur_float4* bounds, const float* hzb_base,
                                const ur_mip_desc* mips, void* indirect_args, uint32_t* stats2, uint32_t* visible_idx,
                                uint32_t* visible_count, uint32_t index_base, const ur_draw_ranges* draws)
{
    return cull_call(ctx, constants, bounds, hzb_base, mips, indirect_args, stats2, visible_idx, visible_count, index_base, draws, nullptr, 0);
}

int ur_cull_indirect_args_views(ur_ctx* ctx, const uint32_t* constants, const ur_float4* bounds, const float* hzb_base,
                                const ur_mip_desc* mips, void* indirect_args, uint32_t* stats2, uint32_t* visible_idx,
                                uint32_t* visible_count, uint32_t index_base, const ur_draw_ranges* draws,
                                const ur_cull_view* views, uint32_t view_count)
{
    return cull_call(ctx, constants, bounds, hzb_base, mips, indirect_args, stats2, visible_idx, visible_count, index_base, draws, views, view_count);
}

} // extern "C"

int ur::check_cull_views(const ur_cull_view* views, uint32_t view_count) { return check_views("ur_frame_set_cull_views", views, view_count, ~0u, nullptr, nullptr); }
