// What every CullIndirectArgs plan must satisfy (csrc/cull_plan.cpp) and the sweep that checks it over the full cross product of the
// recorded sweep's values: shared by tests/cpp/test_cull_plan.cpp and the sanitizer driver tests/cpp/sanitize_main.cpp.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>

#include "../../unclerenderer_amd/csrc/cull_plan.h"

namespace cull_sweep {

static int g_fail = 0;
#define CULL_CHECK(c, ...) do { if (!(c)) { std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); ++cull_sweep::g_fail; } } while (0)

inline void check_plan(const ur::CullPlanInput& in)
{
    const ur::CullPlan p = ur::plan_cull(in);
    const uint32_t n = in.n;
    bool view_compaction = false;
    for (uint32_t v = 0; v < in.view_count; ++v) view_compaction = view_compaction || in.view_compacted[v];
    const bool wants = in.camera_list || in.camera_ranges || view_compaction;
    // the kind, from n alone but for the zeroing launch
    const ur::CullPlan::Kind kind = n == 0 ? (wants ? ur::CullPlan::zero : ur::CullPlan::nothing) : n <= 256u ? ur::CullPlan::single_block : ur::CullPlan::multi_block;
    CULL_CHECK(p.kind == kind, "n %u: kind %d, expected %d", n, (int)p.kind, (int)kind);
    const bool multi = p.kind == ur::CullPlan::multi_block;
    CULL_CHECK(p.blocks == (n + 255u) / 256u && (p.blocks > 1u) == multi, "n %u: %u blocks", n, p.blocks);
    if (p.kind == ur::CullPlan::zero) CULL_CHECK(p.zero_grid >= 1u && (uint64_t)p.zero_grid * 256u >= in.most_ranges && ((uint64_t)p.zero_grid - 1u) * 256u < std::max(1u, in.most_ranges), "%u ranges on %u workgroups", in.most_ranges, p.zero_grid);
    if (n != 0) CULL_CHECK(p.ranges == in.camera_ranges, "n %u: the RANGES instantiation", n);
    // a stop that is armed is carried by exactly one step whenever any step is launched, and by the last one
    const int launches = p.kind == ur::CullPlan::nothing ? 0 : multi && p.compact ? 2 : 1;
    const ur::CullPlan::StopOn last = launches == 0 ? ur::CullPlan::none : !multi ? ur::CullPlan::only : p.compact ? ur::CullPlan::compaction : ur::CullPlan::cull;
    CULL_CHECK(p.stop_on == (in.stop_armed ? last : ur::CullPlan::none) && p.carried() == (in.stop_armed && launches != 0), "n %u: %d launches, stop on %d", n, launches, (int)p.stop_on);
    // the compaction: above one block, for the camera's list or ranges or a compacted view
    CULL_CHECK(p.compact == (p.blocks > 1u && wants), "n %u: compact %d", n, (int)p.compact);
    if (p.compact) CULL_CHECK(p.compact_grid_x == (p.blocks + 63u) / 64u && p.compact_grid_y == 1u + in.view_count, "n %u: compaction grid %u x %u", n, p.compact_grid_x, p.compact_grid_y);
    // the workspace: whoever compacts, has views or keeps a record, above one block; grown to hold n, never shrunk
    CULL_CHECK(p.needs_workspace == (multi && (p.compact || in.view_count != 0 || in.store_flavour == 4u)), "n %u: workspace %d", n, (int)p.needs_workspace);
    CULL_CHECK(p.reserve_to == (p.needs_workspace && n > in.ws_instances ? n : 0u), "n %u over %u: reserve %u", n, in.ws_instances, p.reserve_to);
    CULL_CHECK(p.ws_instances == (p.reserve_to ? (n + 255u) / 256u * 256u : in.ws_instances), "n %u over %u: workspace of %u", n, in.ws_instances, p.ws_instances);
    if (p.needs_workspace) CULL_CHECK(p.ws_instances >= n && p.stride == p.ws_instances / 256u && p.stride >= p.blocks, "n %u: %u blocks in a stride of %u", n, p.blocks, p.stride);
    // slices: compacted views only, pairwise disjoint and disjoint from slice 0 (each holds `blocks` counts from slice * stride), inside
    // the (1 + UR_MAX_CULL_VIEWS) * stride counts ur_reserve allocates
    for (uint32_t v = 0; v < UR_MAX_CULL_VIEWS; ++v) {
        const bool has = p.view_slice[v] >= 0;
        CULL_CHECK(has == (multi && v < in.view_count && in.view_compacted[v]), "n %u view %u: slice %d", n, v, (int)p.view_slice[v]);
        if (!has) continue;
        const uint64_t first = (uint64_t)p.view_slice[v] * p.stride, end = first + p.blocks;
        CULL_CHECK(first >= p.blocks && end <= (uint64_t)(1u + UR_MAX_CULL_VIEWS) * p.stride, "n %u view %u: counts [%llu, %llu) of %u slices of %u", n, v, (unsigned long long)first, (unsigned long long)end, 1u + UR_MAX_CULL_VIEWS, p.stride);
        for (uint32_t u = 0; u < v; ++u) {
            if (p.view_slice[u] < 0) continue;
            const uint64_t f2 = (uint64_t)p.view_slice[u] * p.stride, e2 = f2 + p.blocks;
            CULL_CHECK(end <= f2 || e2 <= first, "n %u: views %u and %u share counts", n, u, v);
        }
    }
    // the record of flavour 4
    if (p.record_valid) CULL_CHECK(in.store_flavour == 4u && in.record_same_buffer && in.record_same_count && p.blocks > 1u && p.reserve_to == 0u, "n %u: a valid record", n);
    else if (multi) CULL_CHECK(!(in.store_flavour == 4u && in.record_same_buffer && in.record_same_count && p.reserve_to == 0u), "n %u: a record not used", n);
    CULL_CHECK(p.keep_record == (in.store_flavour == 4u && p.blocks > 1u), "n %u flavour %u: keep %d", n, in.store_flavour, (int)p.keep_record);
}

// The recorded sweep's values (tests/golden/cull_plans.txt), as a full cross product. Returns the plans made.
inline long sweep()
{
    const uint32_t ns[] = {0, 1, 255, 256, 257, 512, 513, 16384, 16385, 70000, 1000000};
    const uint32_t views[][2] = {{0, 0}, {1, 1}, {1, 0}, {2, 2}, {2, 1}, {4, 15}, {4, 0}, {4, 10}}; // count, compacted bits
    const uint32_t most[] = {0, 1, 256, 257, 70000, 0xFFFFFFFFu};
    long plans = 0;
    for (uint32_t n : ns)
        for (int cam = 0; cam < 4; ++cam)
            for (auto& vw : views)
                for (uint32_t flavour : {0u, 3u, 4u})
                    for (int rec = 0; rec < 4; ++rec)
                        for (int w = 0; w < 3; ++w)
                            for (int stop = 0; stop < 2; ++stop)
                                for (uint32_t m : most) {
                                    if (m != 0 && n != 0 && m != 257u) continue; // (the range count matters to the zeroing launch only)
                                    ur::CullPlanInput in{};
                                    in.n = n;
                                    in.camera_list = (cam & 1) != 0; in.camera_ranges = (cam & 2) != 0;
                                    in.view_count = vw[0];
                                    for (uint32_t v = 0; v < vw[0]; ++v) in.view_compacted[v] = ((vw[1] >> v) & 1u) != 0;
                                    in.most_ranges = m;
                                    in.store_flavour = flavour;
                                    in.record_same_buffer = (rec & 1) != 0; in.record_same_count = (rec & 2) != 0;
                                    const uint32_t exact = (uint32_t)((((uint64_t)n + 255u) / 256u) * 256u);
                                    in.ws_instances = w == 0 ? 0u : w == 1 ? exact : std::max(1u << 20, exact + 4096u);
                                    in.stop_armed = stop != 0;
                                    check_plan(in);
                                    ++plans;
                                }
    return plans;
}

} // namespace cull_sweep
