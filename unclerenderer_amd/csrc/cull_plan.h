// Host decisions of CullIndirectArgs that need no device: which launches one cull call takes, on which grids, who gets the context's
// workspace and whether it grows, where each view's slice of it lies, when the UR_OPT_CULL_STORE = 4 record is valid and when it is kept,
// and which dispatch carries ur_time_next_cull's event. Plain C++17 (no HIP header, no ur_ctx), so a test drives it without a GPU
// (tests/cpp/test_cull_plan.cpp). A plan holds counts, indices and flags only, never pointers: csrc/cull_launch.h binds it to buffers and
// kernels. Not installed.
#pragma once

#include <cstdint>

#include "../../include/ur_hotpath.h"

namespace ur {

struct CullPlanInput {
    uint32_t n;                                // ModelCount
    bool camera_list, camera_ranges;           // the camera has a visible list / draw ranges
    uint32_t view_count;                       // 0 .. UR_MAX_CULL_VIEWS
    bool view_compacted[UR_MAX_CULL_VIEWS];    // the view has a list or ranges (a mask alone needs no compaction)
    uint32_t most_ranges;                      // n == 0 only: the largest range_count among the camera's and the views' ranges (0: none)
    uint32_t store_flavour;                    // UR_OPT_CULL_STORE
    bool record_same_buffer, record_same_count; // the context's record against this call's command buffer and count
    uint32_t ws_instances;                     // the context's workspace, in instances
    bool stop_armed;                           // ur_time_next_cull armed an event
};

struct CullPlan {
    enum Kind : uint8_t {
        nothing,      // n == 0 and no count to zero: no launch
        zero,         // n == 0: zero_views_kernel on zero_grid workgroups
        single_block, // n <= 256: cull_kernel<true, ranges> alone
        multi_block   // cull_kernel<false, ranges> on `blocks` workgroups, then compact_kernel<ranges> when `compact`
    } kind;
    enum StopOn : uint8_t { none, only, cull, compaction } stop_on; // the launch whose dispatch carries the event: the call's last
    bool ranges;          // the RANGES instantiation (arguments with the camera's ranges) against the one without
    bool compact;
    bool needs_workspace; // the cull writes wave masks and block counts: the compaction's input, flavour 4's record
    bool record_valid;    // as passed to the kernel: the workspace holds the visible bits the command buffer has now
    bool keep_record;     // after the last launch the context's record names this buffer and count
    uint32_t zero_grid;
    uint32_t blocks;
    uint32_t compact_grid_x, compact_grid_y; // y: row 0 the camera's, row 1 + v view v's
    uint32_t reserve_to;   // 0, or the instance count to pass to ur_reserve in front of the launches
    uint32_t ws_instances; // the workspace after that reserve
    uint32_t stride;       // block counts per slice (4x as many masks): ws_instances / 256; 0 without a workspace
    int8_t view_slice[UR_MAX_CULL_VIEWS]; // 1 + v for a compacted view of a multi-block call (slice 0 is the camera's), else -1

    bool carried() const { return stop_on != none; } // what ur_time_cull_carried answers after the call
};

CullPlan plan_cull(const CullPlanInput& in);

} // namespace ur
