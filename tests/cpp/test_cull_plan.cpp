// csrc/cull_plan.cpp without a device: the launches cull_launches decided before the planner was split out of it
// (tests/golden/cull_plans.txt), and the invariants of cull_plan_sweep.h over the full cross product of the recorded sweep's values.
//
//   g++ -std=c++17 -O1 -g -Wall tests/cpp/test_cull_plan.cpp unclerenderer_amd/csrc/cull_plan.cpp
#include <fstream>
#include <sstream>
#include <string>

#include "cull_plan_sweep.h"

// A plan in the golden file's words (its header gives the row format)
static std::string words(const ur::CullPlan& p)
{
    static const char* const stop_on[] = {"none", "only", "cull", "compaction"};
    char b[400];
    const int keep = p.keep_record ? 1 : 0, carried = p.carried() ? 1 : 0;
    switch (p.kind) {
    case ur::CullPlan::nothing: std::snprintf(b, sizeof b, " nothing keep %d carried %d", keep, carried); return b;
    case ur::CullPlan::zero: std::snprintf(b, sizeof b, " zero grid %u stop %s keep %d carried %d", p.zero_grid, stop_on[p.stop_on], keep, carried); return b;
    case ur::CullPlan::single_block: std::snprintf(b, sizeof b, " single ranges %d stop %s keep %d carried %d", (int)p.ranges, stop_on[p.stop_on], keep, carried); return b;
    case ur::CullPlan::multi_block: break;
    }
    std::snprintf(b, sizeof b, " multi ranges %d blocks %u compact %d grid %u %u workspace %d reserve %u ws %u stride %u slices", (int)p.ranges, p.blocks, (int)p.compact,
                  p.compact_grid_x, p.compact_grid_y, (int)p.needs_workspace, p.reserve_to, p.ws_instances, p.stride);
    std::string out = b;
    for (uint32_t v = 0; v < UR_MAX_CULL_VIEWS; ++v) out += p.view_slice[v] < 0 ? " -" : " " + std::to_string((int)p.view_slice[v]);
    std::snprintf(b, sizeof b, " valid %d keep %d stop %s carried %d", (int)p.record_valid, keep, stop_on[p.stop_on], carried);
    return out + b;
}

static int golden(const char* path)
{
    std::ifstream f(path);
    CULL_CHECK(f.good(), "cannot open %s", path);
    int rows = 0;
    for (std::string line; std::getline(f, line);) {
        if (line.empty() || line[0] == '#') continue;
        const size_t bar = line.find(" |");
        const std::string head = line.substr(0, bar), want = bar == std::string::npos ? "" : line.substr(bar + 2);
        std::istringstream in(head);
        std::string word;
        ur::CullPlanInput I{};
        uint32_t list = 0, ranges = 0, bits = 0, same_buffer = 0, same_count = 0, stop = 0;
        in >> word >> I.n >> word >> list >> word >> ranges >> word >> I.view_count >> word >> bits >> word >> I.most_ranges >> word >> I.store_flavour >> word >> same_buffer >>
            same_count >> word >> I.ws_instances >> word >> stop;
        CULL_CHECK(!in.fail() && word == "stop" && I.view_count <= UR_MAX_CULL_VIEWS, "unreadable row: %s", line.c_str());
        if (in.fail() || I.view_count > UR_MAX_CULL_VIEWS) continue;
        I.camera_list = list != 0; I.camera_ranges = ranges != 0;
        for (uint32_t v = 0; v < I.view_count; ++v) I.view_compacted[v] = ((bits >> v) & 1u) != 0;
        I.record_same_buffer = same_buffer != 0; I.record_same_count = same_count != 0;
        I.stop_armed = stop != 0;
        const std::string got = words(ur::plan_cull(I));
        CULL_CHECK(got == want, "%s: planned \"%s\", the launch path did \"%s\"", head.c_str(), got.c_str(), want.c_str());
        ++rows;
    }
    return rows;
}

// The calls the GPU tests and the documents name, worked by hand from the rules
static void by_hand()
{
    ur::CullPlanInput I{};
    I.n = 257; I.camera_list = I.camera_ranges = true; I.view_count = 4; I.store_flavour = 4;
    for (bool& c : I.view_compacted) c = true;
    // a workspace that was never reserved: 512 instances, two blocks in a stride of two, every slice exactly full
    ur::CullPlan p = ur::plan_cull(I);
    CULL_CHECK(words(p) == " multi ranges 1 blocks 2 compact 1 grid 1 5 workspace 1 reserve 257 ws 512 stride 2 slices 1 2 3 4 valid 0 keep 1 stop none carried 0", "257 on no workspace: %s", words(p).c_str());
    // the same call again: the record is valid
    I.ws_instances = 512; I.record_same_buffer = I.record_same_count = true; I.stop_armed = true;
    p = ur::plan_cull(I);
    CULL_CHECK(p.record_valid && p.reserve_to == 0u && p.stop_on == ur::CullPlan::compaction, "257 again: %s", words(p).c_str());
    // 16385 on it: 65 blocks, two compaction workgroups per row, the workspace grows and the (other count's) record is not used
    I.n = 16385; I.record_same_count = false;
    p = ur::plan_cull(I);
    CULL_CHECK(p.blocks == 65u && p.compact_grid_x == 2u && p.reserve_to == 16385u && p.ws_instances == 16640u && p.stride == 65u && !p.record_valid && p.keep_record, "16385: %s", words(p).c_str());
    // the frame's own cull: 25 commands, one launch that carries the event; flavour 4 keeps no record of a single block
    ur::CullPlanInput F{};
    F.n = 25; F.camera_list = true; F.store_flavour = 4; F.stop_armed = true; F.ws_instances = 1u << 20;
    p = ur::plan_cull(F);
    CULL_CHECK(words(p) == " single ranges 0 stop only keep 0 carried 1", "25 commands: %s", words(p).c_str());
}

int main(int argc, char** argv)
{
    if (argc < 2) { std::printf("usage: test_cull_plan tests/golden/cull_plans.txt\n"); return 2; }
    const int rows = golden(argv[1]);
    by_hand();
    const long plans = cull_sweep::sweep();
    if (cull_sweep::g_fail) { std::printf("%d check(s) failed\n", cull_sweep::g_fail); return 1; }
    std::printf("OK cull plan: %d recorded calls, %ld swept plans\n", rows, plans);
    return 0;
}
