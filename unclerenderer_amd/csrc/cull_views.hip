// CullIndirectArgs with extra views (ur_cull_indirect_args_views): cull_launches<true> instantiates cull_kernel / compact_kernel with VIEWS
// (cull_kernels.h, launched by cull_launch.h). A translation unit of its own, so that the camera-only kernels in cull.hip compile exactly as they did without views.

#include "cull_kernels.h"
#include "cull_launch.h"

namespace ur {

int launch_cull_views(ur_ctx* ctx, const uint32_t* constants, const ur_float4* bounds, const float* hzb, const ur_mip_desc* mips,
                      void* indirect_args, uint32_t* stats2, uint32_t* visible_idx, uint32_t* visible_count, uint32_t index_base,
                      const ur_draw_ranges* draws, const ur_cull_view* views, uint32_t view_count)
{
    return cull_launches<true>(ctx, constants, bounds, hzb, mips, indirect_args, stats2, visible_idx, visible_count, index_base, draws, views, view_count);
}

} // namespace ur
