// What every Build HZB plan must satisfy (csrc/hzb_plan.cpp), the sweep that checks it and the hostile inputs the planner refuses:
// shared by tests/cpp/test_hzb_plan.cpp and the sanitizer driver tests/cpp/sanitize_main.cpp.
#pragma once

#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../../unclerenderer_amd/csrc/hzb_plan.h"

namespace hzb_sweep {

static int g_fail = 0;
#define HZB_CHECK(c, ...) do { if (!(c)) { std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); ++hzb_sweep::g_fail; } } while (0)

// a w x h depth buffer's chain in an exact-size heap buffer: a read past its end is a sanitizer report
inline std::vector<ur_mip_desc> chain_of(uint32_t w, uint32_t h, uint32_t* total = nullptr)
{
    ur_mip_desc mips[UR_MAX_HZB_MIPS];
    uint32_t count = 0;
    const uint32_t t = ur::hzb_layout(w, h, mips, &count);
    if (total) *total = t;
    return t ? std::vector<ur_mip_desc>(mips, mips + count) : std::vector<ur_mip_desc>();
}

inline void check_chain(uint32_t w, uint32_t h, const std::vector<ur_mip_desc>& mips, int mode, bool can_hold_wide)
{
    const uint32_t count = (uint32_t)mips.size();
    const ur::HzbPlan p = ur::plan_hzb_chain(w, h, mips.data(), count, mode, can_hold_wide);
    HZB_CHECK(p.status == ur::HzbPlan::ok && p.count >= 1u && p.count <= ur::kMaxHzbSteps, "%u x %u mode %d: status %d, %u steps", w, h, mode, (int)p.status, p.count);
    const bool wide_plus_tail = ur::hzb_chain_is_wide_plus_tail(mips.data(), count);
    uint32_t next = 0;
    for (uint32_t i = 0; i < p.count; ++i) {
        const ur::HzbStep& s = p.steps[i];
        // every level exactly once, in ascending order
        HZB_CHECK(s.first == next && s.levels >= 1u, "%u x %u mode %d step %u: first %u levels %u behind level %u", w, h, mode, i, s.first, s.levels, next);
        next = s.first + s.levels;
        if (next > count) break;
        if (s.kind == ur::HzbStep::wide) {
            HZB_CHECK(s.levels <= (i == 0 ? 5u : 4u), "%u x %u step %u: a wide step of %u levels", w, h, i, s.levels);
            HZB_CHECK(s.from_depth == (i == 0), "%u x %u step %u: source", w, h, i);
            HZB_CHECK(s.grid_x == (mips[s.first].width + 63u) / 64u && s.grid_y == (mips[s.first].height + 15u) / 16u && s.by0 == 0u, "%u x %u step %u: grid %u x %u", w, h, i, s.grid_x, s.grid_y);
            // mode 0 holds nothing, mode 1 the tail only, mode 2 the wide step only of a chain that is wide plus tail
            HZB_CHECK(!s.hold || (mode == 2 && can_hold_wide && wide_plus_tail && i == 0 && s.levels == 5u), "%u x %u mode %d step %u: held", w, h, mode, i);
            if (mode == 2 && can_hold_wide && wide_plus_tail) HZB_CHECK(s.hold && p.count == 2u, "%u x %u: mode 2 launches the wide step of a wide-plus-tail chain", w, h);
        } else {
            HZB_CHECK(i > 0 && i + 1u == p.count && !s.from_depth, "%u x %u step %u: a tail that is not the last step behind a wide one", w, h, i);
            HZB_CHECK((uint64_t)mips[s.first].width * mips[s.first].height <= ur::kTailTexels && s.levels <= ur::kTailMaxLevels, "%u x %u: tail from level %u, %u levels", w, h, s.first, s.levels);
            HZB_CHECK(s.hold == (mode != 0), "%u x %u mode %d: tail %s", w, h, mode, s.hold ? "held" : "launched");
        }
    }
    HZB_CHECK(next == count, "%u x %u mode %d: levels up to %u of %u", w, h, mode, next, count);
    if (wide_plus_tail) HZB_CHECK(p.count == 2u && p.steps[0].levels == 5u && p.steps[1].kind == ur::HzbStep::tail && p.steps[1].first == 5u, "%u x %u: wide plus tail", w, h);
}

// Every w, h in 1..200 and a few hundred random sizes up to 65536 x 8192, every mode, with and without the arrival counter. Returns the plans made.
inline long sweep()
{
    long plans = 0;
    auto one = [&](uint32_t w, uint32_t h) {
        const std::vector<ur_mip_desc> mips = chain_of(w, h);
        HZB_CHECK(!mips.empty(), "%u x %u: no layout", w, h);
        if (mips.empty()) return;
        for (int mode = 0; mode <= 2; ++mode)
            for (int can = 0; can <= 1; ++can, ++plans) check_chain(w, h, mips, mode, can != 0);
    };
    for (uint32_t w = 1; w <= 200; ++w)
        for (uint32_t h = 1; h <= 200; ++h) one(w, h);
    std::mt19937 rng(5);
    for (int k = 0; k < 400; ++k) {
        const uint32_t w = 1u + rng() % 65536u, h = 1u + rng() % 8192u;
        one(w, h);
        one(h, w > 8192u ? 1u + w % 8192u : w);
    }
    for (uint32_t w : {65535u, 65536u})
        for (uint32_t h : {1u, 2u, 8191u, 8192u}) one(w, h);
    return plans;
}

// Hostile inputs: each is refused, and (under the sanitizers, on exact-size buffers) never read past its end. Returns the refusals.
inline int hostile()
{
    int refused = 0;
    auto expect_invalid = [&](const char* what, uint32_t w, uint32_t h, const ur_mip_desc* mips, uint32_t count) {
        for (int mode = 0; mode <= 2; ++mode) {
            const ur::HzbPlan a = ur::plan_hzb_chain(w, h, mips, count, mode), b = ur::plan_hzb_band(w, h, mips, count, mode, 0u, 1u);
            HZB_CHECK(a.status == ur::HzbPlan::invalid_chain && a.count == 0u && b.status == ur::HzbPlan::invalid_chain && b.count == 0u, "%s: mode %d", what, mode);
            ++refused;
        }
    };
    const std::vector<ur_mip_desc> good = chain_of(3840, 2160);
    expect_invalid("no mips", 3840, 2160, nullptr, 11);
    expect_invalid("mip_count 0", 3840, 2160, good.data(), 0);
    {
        std::vector<ur_mip_desc> seventeen(17, good[0]); // (17 real entries: a planner that walked them would find nothing to fault on)
        expect_invalid("mip_count 17", 3840, 2160, seventeen.data(), 17);
        HZB_CHECK(ur::plan_hzb_tail(seventeen.data(), 17).status == ur::HzbPlan::invalid_chain, "tail of 17 levels");
    }
    expect_invalid("zero width", 0, 2160, good.data(), (uint32_t)good.size());
    expect_invalid("zero height", 3840, 0, good.data(), (uint32_t)good.size());
    expect_invalid("another frame's chain", 3838, 2160, good.data(), (uint32_t)good.size());
    for (size_t m = 0; m < good.size(); ++m) { // a chain that does not halve, at every level
        std::vector<ur_mip_desc> bad = good;
        bad[m].width += 1u;
        expect_invalid("does not halve", 3840, 2160, bad.data(), (uint32_t)bad.size());
        // (the tail form knows no source size: mips[0] is what it is, the levels below it halve from it)
        if (m != 0) HZB_CHECK(ur::plan_hzb_tail(bad.data(), (uint32_t)bad.size()).status == ur::HzbPlan::invalid_chain, "tail of a chain that does not halve at %zu", m);
        bad = good;
        bad[m].height = 0u;
        expect_invalid("a level of no rows", 3840, 2160, bad.data(), (uint32_t)bad.size());
    }
    for (uint32_t n = 1; n < good.size(); ++n) { // a chain cut short is a valid shorter chain or refused: its exact-size copy is never read past n
        const std::vector<ur_mip_desc> cut(good.begin(), good.begin() + n);
        const ur::HzbPlan p = ur::plan_hzb_chain(3840, 2160, cut.data(), n, 2);
        HZB_CHECK(p.status == ur::HzbPlan::ok, "the first %u levels", n);
        if (p.status == ur::HzbPlan::ok) check_chain(3840, 2160, cut, 2, true);
        (void)ur::plan_hzb_band(3840, 2160, cut.data(), n, 2, 0u, 68u);
        (void)ur::plan_hzb_tail(cut.data(), n);
    }
    HZB_CHECK(ur::plan_hzb_tail(nullptr, 11).status == ur::HzbPlan::invalid_chain && ur::plan_hzb_tail(good.data(), 0).status == ur::HzbPlan::invalid_chain, "tail: null / empty");
    {
        std::vector<ur_mip_desc> overlap = good;
        overlap[6].offset = overlap[5].offset; // (the tail form takes a chain below mips[0]: its levels must not overlap)
        HZB_CHECK(ur::plan_hzb_tail(overlap.data(), (uint32_t)overlap.size()).status == ur::HzbPlan::invalid_chain, "tail: overlapping levels");
    }
    return refused;
}

} // namespace hzb_sweep
