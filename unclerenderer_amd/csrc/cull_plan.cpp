// The launches of one CullIndirectArgs call (cull_plan.h): integer arithmetic on plain values, no allocation.
#include "cull_plan.h"

#include <algorithm>

namespace ur {

CullPlan plan_cull(const CullPlanInput& in)
{
    CullPlan p{};
    for (int8_t& s : p.view_slice) s = -1;
    p.ws_instances = in.ws_instances;
    // (defensive only, no decision of the launch path: the entry point refuses more views, and the per-view arrays here hold no more)
    const uint32_t view_count = std::min<uint32_t>(in.view_count, UR_MAX_CULL_VIEWS);
    bool view_compaction = false;
    for (uint32_t v = 0; v < view_count; ++v) view_compaction = view_compaction || in.view_compacted[v];
    const CullPlan::StopOn last_of_one = in.stop_armed ? CullPlan::only : CullPlan::none;

    if (in.n == 0) { // one launch zeroes every count and every counts[r], if there are any (no mask word is written)
        if (!in.camera_list && !in.camera_ranges && !view_compaction) return p; // (kind nothing: the event is not carried)
        p.kind = CullPlan::zero;
        p.zero_grid = std::max(1u, (uint32_t)(((uint64_t)in.most_ranges + 255u) / 256u));
        p.stop_on = last_of_one;
        return p;
    }
    p.ranges = in.camera_ranges;
    p.blocks = (in.n + 255u) / 256u; // (32-bit, as the launch always computed it)
    if (p.blocks == 1) {             // (one block keeps no masks: no record, no workspace)
        p.kind = CullPlan::single_block;
        p.stop_on = last_of_one;
        return p;
    }
    p.kind = CullPlan::multi_block;
    // the compaction follows when there is a list or there are ranges, the camera's or a view's
    p.compact = in.camera_list || in.camera_ranges || view_compaction;
    // the masks and block counts: the compaction's input, flavour 4's record (with views the camera's are always written)
    p.needs_workspace = view_count != 0 || p.compact || in.store_flavour == 4u;
    // UR_OPT_CULL_STORE = 4: the wave masks ARE the record of what a multi-block launch leaves in the command buffer; they describe the
    // buffer this launch meets if it is on the same buffer with the same count
    p.record_valid = in.store_flavour == 4u && in.record_same_buffer && in.record_same_count;
    if (p.needs_workspace) {
        if (in.n > in.ws_instances) {
            p.reserve_to = in.n;
            p.ws_instances = (uint32_t)((((uint64_t)in.n + 255u) / 256u) * 256u); // what ur_reserve leaves
            // A new workspace holds no record. (Unreachable as long as a record is only kept by a call whose workspace held n
            // instances and the workspace never shrinks: kept because the launch path always had it.)
            p.record_valid = false;
        }
        p.stride = p.ws_instances / 256u;
        for (uint32_t v = 0; v < view_count; ++v)
            if (in.view_compacted[v]) p.view_slice[v] = (int8_t)(1u + v);
    }
    p.compact_grid_x = (p.blocks * 4u + 255u) / 256u;
    p.compact_grid_y = 1u + view_count;
    p.keep_record = in.store_flavour == 4u;
    if (in.stop_armed) p.stop_on = p.compact ? CullPlan::compaction : CullPlan::cull;
    return p;
}

} // namespace ur
