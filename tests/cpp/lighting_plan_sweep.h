// Invariants of csrc/lighting_plan.cpp over a sweep of devices, bands and options: what the streaming kernel and its launch rely on.
// Shared by tests/cpp/test_lighting_plan.cpp and the sanitizer driver (tests/cpp/sanitize_main.cpp), which runs it under ASan/UBSan.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>

#include "../../unclerenderer_amd/csrc/lighting_plan.h"

namespace plan_sweep {

inline int g_fail = 0;
#define PLAN_CHECK(c, ...)                                                      \
    do {                                                                        \
        if (!(c)) {                                                             \
            if (++plan_sweep::g_fail <= 20) { std::printf("FAIL %s:%d %s  ", __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                       \
    } while (0)

inline void check_magic(const ur::StreamPlan& s, uint32_t tile)
{
    PLAN_CHECK((uint32_t)(((uint64_t)tile * s.tilesXMagic) >> 32) == tile / s.tilesX, "tile %u of %u, tilesX %u", tile, s.numTiles, s.tilesX);
}

// One plan against its input
inline void check_plan(const ur::StreamPlanInput& in, const ur::StreamPlan& s)
{
    const int cus = std::max(in.cus, 1), leave = std::min(in.leave_cus, cus - 1);
    const uint32_t left = (uint32_t)std::max(1, cus - (s.carry_tail ? 1 : 0) - leave); // the CUs left to lighting
    PLAN_CHECK(s.tilesX == in.W / 16u && s.numTiles == s.tilesX * ((in.rows + 3u) / 4u), "W %u rows %u", in.W, in.rows);
    PLAN_CHECK(s.groups >= 1u && s.groups <= left, "groups %u of %u (cus %d leave %d)", s.groups, left, in.cus, in.leave_cus);
    // the same bound from the device's side: the launch's workgroups never outnumber the CUs, and what was asked to be left is left while one CU remains for lighting
    PLAN_CHECK((int)(s.groups + (s.carry_tail ? 1u : 0u)) <= cus, "%u workgroups on %d CUs", s.groups + (s.carry_tail ? 1u : 0u), cus);
    if (in.leave_cus >= 0 && in.leave_cus < cus && s.groups > 1u) PLAN_CHECK((int)(s.groups + (s.carry_tail ? 1u : 0u)) + in.leave_cus <= cus, "leave %d of %d", in.leave_cus, cus);
    PLAN_CHECK((uint64_t)s.groups * in.wpb < (uint64_t)s.numTiles + in.wpb, "no workgroup without a tile: %u x %u for %u", s.groups, in.wpb, s.numTiles);
    PLAN_CHECK(!s.carry_tail || (in.tail_pending && in.wpb == 16u && cus >= 16 && cus - leave >= 2), "a tail is carried only on a CU of its own");
    PLAN_CHECK(s.ride_want == s.groups + (in.debug_hzb_ride_stall != 0 ? 1u : 0u), "want %u", s.ride_want);
    // pieces: ride or go out in front, never both, never lost
    if (in.wide_pending) {
        PLAN_CHECK(s.rides != s.flush_first, "pieces %u flush %d", s.ride_pieces, (int)s.flush_first);
        PLAN_CHECK(s.rides || s.ride_pieces == 0u, "pieces without a ride");
        if (in.wpb != 16u || cus < 16 || (in.tail_pending && !s.carry_tail)) PLAN_CHECK(s.flush_first && !s.rides && s.ride_pieces == 0u, "a launch that cannot ride");
        if (s.rides) {
            PLAN_CHECK(s.ride_pieces == in.wide_grid_x * in.wide_grid_y && s.ride_grid_x == in.wide_grid_x, "pieces %u", s.ride_pieces);
            PLAN_CHECK(s.ride_walkers == 1u || s.ride_walkers == in.wpb, "walkers %u", s.ride_walkers);
            PLAN_CHECK((s.ride_spin_limit != 0u) == s.carry_tail, "only a carried tail waits");
            if (in.ride_walkers >= 1) PLAN_CHECK(s.ride_walkers == (in.ride_walkers >= 4 ? in.wpb : 1u), "forced %d -> %u", in.ride_walkers, s.ride_walkers);
        }
    } else {
        PLAN_CHECK(!s.rides && s.ride_pieces == 0u && !s.flush_first && s.ride_walkers == 0u, "nothing pending, nothing rides");
    }
    PLAN_CHECK(s.reported[0] == s.groups && s.reported[1] == s.numTiles && s.reported[3] == s.poolChunks && s.reported[4] == s.dynShift &&
               s.reported[5] == s.lookahead && s.reported[6] == in.wpb && s.reported[7] == s.ride_pieces, "the reported words");
    if (s.poolChunks == 0u) {
        PLAN_CHECK(s.staticClaims == 0xFFFFFFFFu && s.reported[2] == s.numTiles && s.staticTiles == 0u && s.dynShift == 0u && s.lookahead == 0u && s.poolMagic == 0u, "all static");
        return;
    }
    // a pool exists
    PLAN_CHECK(in.balance != 0 && in.claim_words != 0u && s.groups >= 16u && s.groups <= 8u * in.claim_words, "groups %u", s.groups);
    PLAN_CHECK(s.dynShift == (uint32_t)in.balance_chunk_shift && s.lookahead == (s.dynShift >= 4u ? 2u : s.dynShift == 3u ? 3u : 4u), "shift %u ahead %u", s.dynShift, s.lookahead);
    PLAN_CHECK(s.reported[2] == s.staticTiles && s.staticTiles < s.numTiles, "static %u of %u", s.staticTiles, s.numTiles);
    // the static part: whole rounds of the static deal, the two tiles of every wave's prologue among them
    PLAN_CHECK(s.staticTiles == s.staticClaims * s.groups && s.staticClaims % (1u << ur::kChunkShift) == 0u && s.staticClaims >= 2u * in.wpb, "claims %u", s.staticClaims);
    // the pool covers the rest and does not overshoot by a full chunk
    const uint64_t covered = (uint64_t)s.staticTiles + ((uint64_t)s.poolChunks << s.dynShift);
    PLAN_CHECK(covered >= s.numTiles && covered - s.numTiles < (1ull << s.dynShift), "static %u + %u << %u for %u", s.staticTiles, s.poolChunks, s.dynShift, s.numTiles);
    // the requested pool is the least the run-time part holds, and it holds less than one round more
    const uint64_t want_pool = (uint64_t)s.numTiles * (uint32_t)in.balance_pool_16ths / 16u;
    PLAN_CHECK(s.numTiles - s.staticTiles >= want_pool && s.numTiles - s.staticTiles - want_pool < ((uint64_t)s.groups << ur::kChunkShift), "pool %u wanted %llu", s.numTiles - s.staticTiles, (unsigned long long)want_pool);
    // every claim word's share: at least `lookahead` chunks per workgroup of its eight, shares in order, no more than the pool in all
    uint32_t prev = 0;
    for (uint32_t q8 = 0; q8 < s.groups; q8 += 8u) {
        const uint32_t nq = std::min(8u, s.groups - q8);
        const uint32_t P0 = (uint32_t)((q8 * s.poolMagic) >> 32), P1 = (uint32_t)(((q8 + nq) * s.poolMagic) >> 32);
        PLAN_CHECK(P0 == prev && P1 >= P0 + s.lookahead * nq && P1 <= s.poolChunks, "word %u: [%u, %u) of %u", q8 / 8u, P0, P1, s.poolChunks);
        // a workgroup's slot table holds its word's whole share: the pre-assigned chunks, the claims, the end mark
        PLAN_CHECK(P1 - P0 + s.lookahead + 1u < ur::kDynSlots, "word %u: %u chunks", q8 / 8u, P1 - P0);
        prev = P1;
    }
    PLAN_CHECK(prev == s.poolChunks, "the shares end at %u of %u", prev, s.poolChunks);
    PLAN_CHECK((uint64_t)s.poolChunks * 8u / s.groups + s.lookahead + 8u <= ur::kDynSlots, "the slot-table bound");
}

inline ur::StreamPlanInput input(int cus, uint32_t W, uint32_t rows, uint32_t wpb)
{
    ur::StreamPlanInput in{};
    in.cus = cus; in.balance = 1; in.balance_pool_16ths = 3; in.balance_chunk_shift = 4;
    in.W = W; in.rows = rows; in.wpb = wpb; in.claim_words = 32;
    return in;
}

// returns the number of plans checked
inline unsigned long long sweep()
{
    unsigned long long n = 0;
    const int cu_counts[] = {1, 2, 15, 16, 17, 32, 256, 257, 304};
    const uint32_t row_counts[] = {1, 4, 7, 270, 540, 1083, 2160};
    for (int cus : cu_counts)
        for (uint32_t W = 32; W <= 4096; W += 16)
            for (uint32_t rows : row_counts)
                for (uint32_t wpb : {16u, 12u}) {
                    ur::StreamPlanInput in = input(cus, W, rows, wpb);
                    {   // the division by multiplication, once per shape: every tile of a small band; the ends and the row starts of a large one
                        const ur::StreamPlan s = ur::plan_stream(in);
                        if (s.numTiles <= 4096u) for (uint32_t t = 0; t < s.numTiles; ++t) check_magic(s, t);
                        else
                            for (uint32_t r : {0u, 1u, 2u, s.numTiles / s.tilesX / 2u, s.numTiles / s.tilesX - 2u, s.numTiles / s.tilesX - 1u})
                                for (uint32_t t : {r * s.tilesX, r * s.tilesX + 1u, (r + 1u) * s.tilesX - 2u, (r + 1u) * s.tilesX - 1u}) check_magic(s, t);
                    }
                    const int leaves[] = {0, 8, cus - 1, cus, cus + 3}; // (UR_OPT_LIGHTING_LEAVE_CUS takes 0 .. 128; the plan keeps one CU whatever it says)
                    for (int leave : leaves) {
                        in.leave_cus = leave;
                        // every pool and chunk size the options accept (they matter from 16 workgroups on), nothing pending
                        for (int pool = 1; pool <= (cus >= 16 ? 8 : 1); ++pool)
                            for (int shift = 2; shift <= (cus >= 16 ? 6 : 2); ++shift) {
                                in.balance_pool_16ths = pool; in.balance_chunk_shift = shift;
                                check_plan(in, ur::plan_stream(in));
                                ++n;
                            }
                        in.balance_pool_16ths = 3; in.balance_chunk_shift = 4;
                        // what may be pending: a tail, the whole chain, a band's pieces; walkers forced or not; the stall option; no claim words; balance off
                        for (int pending = 1; pending < 4; ++pending)
                            for (int forced : {0, 1, 16}) {
                                ur::StreamPlanInput q = in;
                                q.tail_pending = (pending & 1) != 0; q.wide_pending = (pending & 2) != 0;
                                q.wide_grid_x = (W + 127u) / 128u; q.wide_grid_y = (rows + 31u) / 32u;
                                q.ride_walkers = forced; q.debug_hzb_ride_stall = forced == 1;
                                check_plan(q, ur::plan_stream(q));
                                ++n;
                            }
                        ur::StreamPlanInput q = in;
                        q.claim_words = 0;
                        check_plan(q, ur::plan_stream(q));
                        PLAN_CHECK(ur::plan_stream(q).poolChunks == 0u, "no claim words, no pool");
                        q = in;
                        q.balance = 0;
                        PLAN_CHECK(ur::plan_stream(q).poolChunks == 0u, "balance off, no pool");
                        n += 2;
                    }
                }
    return n;
}

} // namespace plan_sweep
