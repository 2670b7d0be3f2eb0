// csrc/lighting_plan.cpp without a device: schedules recorded from launches on an MI355X (tests/golden/lighting_schedules.json, handed
// over by tests/test_lighting_plan_cpp.py as lines of numbers), values worked by hand from the rules, the invariants of
// lighting_plan_sweep.h over a sweep, and the staged cube's layout.
//
//   g++ -std=c++17 -O1 -g -Wall tests/cpp/test_lighting_plan.cpp unclerenderer_amd/csrc/lighting_plan.cpp
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "lighting_plan_sweep.h"

using plan_sweep::input;

// per line: cus leave_cus ride_walkers balance pool_16ths chunk_shift stall W rows wpb tail_pending wide_pending grid_x grid_y claim_words, the eight words
static int recorded(const char* path)
{
    std::FILE* f = std::fopen(path, "r");
    if (!f) { std::printf("FAIL cannot open %s\n", path); ++plan_sweep::g_fail; return 0; }
    int rows = 0;
    for (;;) {
        long long v[23];
        int got = 0;
        while (got < 23 && std::fscanf(f, "%lld", &v[got]) == 1) ++got;
        if (got == 0) break;
        if (got != 23) { std::printf("FAIL %s: a line of %d numbers\n", path, got); ++plan_sweep::g_fail; break; }
        ur::StreamPlanInput in{(int)v[0], (int)v[1], (int)v[2], (int)v[3], (int)v[4], (int)v[5], (int)v[6], (uint32_t)v[7], (uint32_t)v[8], (uint32_t)v[9],
                               v[10] != 0, v[11] != 0, (uint32_t)v[12], (uint32_t)v[13], (uint32_t)v[14]};
        const ur::StreamPlan s = ur::plan_stream(in);
        plan_sweep::check_plan(in, s);
        for (int k = 0; k < 8; ++k)
            PLAN_CHECK(s.reported[k] == (uint32_t)v[15 + k], "recorded launch %d (%u x %u on %d CUs): word %d is %u, the device reported %lld", rows, in.W, in.rows,
                       in.cus, k, s.reported[k], v[15 + k]);
        ++rows;
    }
    std::fclose(f);
    return rows;
}

// The parent's formulas worked by hand for 256 CUs, nothing left out
static void by_hand()
{
    {   // 3840 x 2160 with its whole 30 x 68 chain riding: one CU goes to the tail; 2040 pieces / 255 = 8 per workgroup want 56 tile times,
        // a wave has 129600 / (255 * 16) = 31.8 tiles: two walkers would do, which is below four: the last wave alone
        ur::StreamPlanInput in = input(256, 3840, 2160, 16);
        in.tail_pending = in.wide_pending = true; in.wide_grid_x = 30; in.wide_grid_y = 68;
        const ur::StreamPlan s = ur::plan_stream(in);
        PLAN_CHECK(s.carry_tail && s.groups == 255u && s.numTiles == 129600u && s.ride_pieces == 2040u && s.ride_walkers == 1u && !s.flush_first, "groups %u walkers %u", s.groups, s.ride_walkers);
        PLAN_CHECK(s.ride_want == 255u && s.ride_spin_limit == (1u << 22) && s.tilesX == 240u && s.tilesXMagic == 17895698u, "magic %u", s.tilesXMagic);
        PLAN_CHECK(ur::ride_walkers(2040, 129600, 255, 16, 0) == 1u && ur::ride_walkers(2040, 129600, 255, 16, 4) == 16u, "the rule itself");
        // the default pool: 3/16 of 129600 = 24300 tiles; rounds of 255 * 4 = 1020: (129600 - 24300) / 1020 = 103 -> 105060 static tiles,
        // 24540 tiles in 1534 chunks of 16 (the last one short), two claimed ahead
        PLAN_CHECK(s.staticClaims == 412u && s.staticTiles == 105060u && s.poolChunks == 1534u && s.dynShift == 4u && s.lookahead == 2u, "static %u chunks %u", s.staticTiles, s.poolChunks);
        PLAN_CHECK(s.poolMagic == ((1534ull << 32) + 254u) / 255u, "pool magic");
    }
    {   // a 1920 x 270 band carrying a 15 x 34 chain with its tail: 510 pieces / 255 = 2 per workgroup want 14 tile times, a wave has
        // 8160 / 4080 = 2 tiles: eight walkers, at least four: every wave
        ur::StreamPlanInput in = input(256, 1920, 270, 16);
        in.tail_pending = in.wide_pending = true; in.wide_grid_x = 15; in.wide_grid_y = 34;
        ur::StreamPlan s = ur::plan_stream(in);
        PLAN_CHECK(s.carry_tail && s.groups == 255u && s.numTiles == 8160u && s.ride_pieces == 510u && s.ride_walkers == 16u, "groups %u walkers %u", s.groups, s.ride_walkers);
        PLAN_CHECK(s.poolChunks == 0u && s.staticClaims == 0xFFFFFFFFu, "32 tiles per workgroup: too short for a run-time part");
        // the same pieces without a tail (a band-sharded chain): no CU set aside, the same rule with 256 workgroups, nobody waits
        in.tail_pending = false;
        s = ur::plan_stream(in);
        PLAN_CHECK(!s.carry_tail && s.groups == 256u && s.ride_pieces == 510u && s.ride_walkers == 16u && s.ride_spin_limit == 0u && !s.flush_first, "groups %u walkers %u", s.groups, s.ride_walkers);
        PLAN_CHECK(ur::ride_walkers(510, 8160, 256, 16, 0) == 16u && ur::ride_walkers(510, 8160, 255, 16, 0) == 16u && ur::ride_walkers(510, 8160, 256, 16, 2) == 1u, "the rule itself");
        // the 12-wave build carries nothing: the chain goes out in front, the tail stays pending for whoever flushes it
        in.tail_pending = true; in.wpb = 12;
        s = ur::plan_stream(in);
        PLAN_CHECK(!s.carry_tail && s.flush_first && s.ride_pieces == 0u && s.groups == 256u, "12 waves");
    }
    {   // a pending wide launch of no pieces beside a carried tail is consumed like any other: it rides (nothing to walk), nothing goes out in front
        ur::StreamPlanInput in = input(256, 1920, 1080, 16);
        in.tail_pending = in.wide_pending = true;
        const ur::StreamPlan s = ur::plan_stream(in);
        PLAN_CHECK(s.carry_tail && s.rides && !s.flush_first && s.ride_pieces == 0u && s.ride_walkers == 1u && s.ride_spin_limit == (1u << 22), "an empty grid");
    }
    {   // two tiles, one workgroup
        const ur::StreamPlan s = ur::plan_stream(input(256, 32, 4, 16));
        PLAN_CHECK(s.groups == 1u && s.numTiles == 2u && s.tilesXMagic == 0x80000001u && s.poolChunks == 0u, "32 x 4");
    }
}

static void cube()
{
    // ur_env_cube_texels of the commit before the layout was stated once (taken from that build's library)
    const struct { uint32_t base, mips; uint64_t texels; } want[] = {{256, 9, 1337154}, {1, 1, 108}, {2, 2, 312}, {3, 2, 438}, {256, 16, 1337910}, {4096, 13, 335962602},
                                                                     {16, 5, 6906}, {32, 6, 23940}, {0, 3, 0}, {8, 0, 0}, {8, 17, 0}, {0xFFFFFFFFu, 16, 4292214880ull}, {0xFFFFFFFEu, 1, 0}};
    for (const auto& w : want) {
        const ur::CubeLayout L = ur::cube_layout(w.base, w.mips);
        PLAN_CHECK(L.texels == w.texels, "%u^2, %u mips: %" PRIu64 " texels, not %" PRIu64, w.base, w.mips, L.texels, w.texels);
        PLAN_CHECK((L.mips == 0u) == (w.base == 0u || w.mips == 0u || w.mips > 16u), "refused: %u^2, %u mips", w.base, w.mips);
        if (L.mips == 0u || w.base > 4096u) continue;
        PLAN_CHECK(L.bytes == L.texels * 8u && L.pairs[L.mips] == L.bytes && L.bordered[0] == 0u, "totals");
        for (uint32_t m = 0; m < L.mips; ++m) {
            const uint64_t e = std::max(1u, w.base >> m) + 2u;
            PLAN_CHECK(L.edge[m] == e && L.size(m) == e - 2u, "edge of mip %u", m);
            PLAN_CHECK((m + 1u < L.mips ? L.bordered[m + 1u] : L.pairs[0] / 8u) == L.bordered[m] + 6u * e * e, "bordered faces of mip %u", m);
            PLAN_CHECK(L.pairs[m + 1u] == L.pairs[m] + 6u * e * (e - 1u) * 12u, "row pairs of mip %u", m);
        }
    }
    // the shipped cube: mips 4..8 fit a workgroup's LDS copy (31 968 bytes); a cube whose last mip alone does not fit keeps nothing
    const ur::CubeLayout L = ur::cube_layout(256, 9);
    const uint32_t first = ur::cube_first_mip_within(L, ur::kLdsCubeBytes);
    PLAN_CHECK(first == 4u && L.bytes - L.pairs[first] == 31968u && L.bytes - L.pairs[3] > ur::kLdsCubeBytes, "first %u", first);
    PLAN_CHECK(ur::cube_first_mip_within(L, 431u) == 9u && ur::cube_first_mip_within(L, 432u) == 8u && ur::cube_first_mip_within(L, ~0ull) == 0u, "budgets");
    PLAN_CHECK(L.bytes < (1ull << 24) && ur::cube_layout(512, 10).bytes >= (1ull << 24), "the streaming kernel's fp32 byte offsets: base sizes up to 256");
}

int main(int argc, char** argv)
{
    const int rows = argc > 1 ? recorded(argv[1]) : 0;
    by_hand();
    cube();
    const unsigned long long plans = plan_sweep::sweep();
    if (plan_sweep::g_fail) { std::printf("%d check(s) failed\n", plan_sweep::g_fail); return 1; }
    std::printf("OK lighting plan: %d recorded launches, %llu plans swept\n", rows, plans);
    return 0;
}
