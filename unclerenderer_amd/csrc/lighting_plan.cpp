// The staged cube's layout and the streaming launch's schedule (lighting_plan.h): integer and double arithmetic on plain values.
#include "lighting_plan.h"

#include <algorithm>

namespace ur {

CubeLayout cube_layout(uint32_t base_size, uint32_t mip_count)
{
    CubeLayout L{};
    if (base_size == 0 || mip_count == 0 || mip_count > 16) return L;
    L.mips = mip_count;
    uint64_t texels = 0;
    for (uint32_t m = 0; m < mip_count; ++m) {
        L.edge[m] = std::max(1u, base_size >> m) + 2u; // (32-bit: see CubeLayout::edge)
        L.bordered[m] = texels;
        texels += 6u * L.edge[m] * L.edge[m];
    }
    uint64_t bytes = texels * 8u;
    for (uint32_t m = 0; m < mip_count; ++m) {
        L.pairs[m] = bytes;
        bytes += 6u * L.edge[m] * (L.edge[m] - 1u) * 12u;
        texels += 9u * L.edge[m] * (L.edge[m] - 1u);
    }
    L.pairs[mip_count] = L.bytes = bytes;
    L.texels = texels;
    return L;
}

uint32_t cube_first_mip_within(const CubeLayout& L, uint64_t budget)
{
    uint32_t first = L.mips;
    while (first > 0 && L.bytes - L.pairs[first - 1u] <= budget) --first;
    return first;
}

uint32_t ride_walkers(uint32_t pieces, uint32_t tiles, uint32_t lighting_groups, uint32_t wpb, int forced)
{
    const double per_group = (double)pieces / lighting_groups, tiles_per_wave = (double)tiles / (lighting_groups * wpb);
    uint32_t wk = 1;
    while (wk < wpb && (double)wk * tiles_per_wave < 7.0 * per_group) wk *= 2;
    if (forced >= 1) wk = (uint32_t)forced;
    return wk >= 4u ? wpb : 1u;
}

StreamPlan plan_stream(const StreamPlanInput& in)
{
    StreamPlan s{};
    const uint32_t WPB = in.wpb;
    s.tilesX = in.W / 16u;
    s.numTiles = s.tilesX * ((in.rows + 3u) / 4u);
    // A deferred HZB tail (ur_defer_hzb_tail) rides along as one extra 1024-thread workgroup on a CU of its own: the
    // lighting workgroups give up one CU (0.4 % of their throughput) and the frame saves a ~5 us single-workgroup launch.
    // UR_OPT_LIGHTING_LEAVE_CUS = n leaves n CUs to kernels of other streams (the graph's async-compute passes): the persistent
    // workgroups otherwise fill every CU's register file and nothing runs beside them. Never below one lighting workgroup
    // (a CPX partition reports 32 CUs), and the tail is carried only when that still leaves the lighting a CU of its own.
    const int cus = std::max(in.cus, 1);
    const int leave_cus = std::min(in.leave_cus, cus - 1);
    const bool can_ride = WPB == 16u && cus >= 16; // (the 12-wave build and a tiny device carry nothing)
    s.carry_tail = in.tail_pending && can_ride && cus - leave_cus >= 2;
    // Pieces ride beside a carried tail (the whole chain: the lighting workgroups take the wide launch's pieces along), or without any
    // tail pending: a band-sharded chain's (ur_build_hzb_band), whose tail waits for the ranks' gather. Nothing inside that launch
    // consumes the pieces, so no arrival is signalled and no CU is set aside.
    s.rides = in.wide_pending && (s.carry_tail || (!in.tail_pending && can_ride));
    if (s.rides) {
        s.ride_grid_x = in.wide_grid_x;
        s.ride_pieces = in.wide_grid_x * in.wide_grid_y;
        if (s.carry_tail) s.ride_spin_limit = in.debug_hzb_ride_stall != 0 ? (1u << 9) : (1u << 22);
        s.ride_walkers = ride_walkers(s.ride_pieces, s.numTiles, (uint32_t)std::max(1, cus - (s.carry_tail ? 1 : 0) - leave_cus), WPB, in.ride_walkers);
    } else {
        s.flush_first = in.wide_pending;
    }
    const uint32_t groups = std::min<uint32_t>((uint32_t)std::max(1, cus - (s.carry_tail ? 1 : 0) - leave_cus), (s.numTiles + WPB - 1) / WPB);
    s.groups = groups;
    s.ride_want = groups + (in.debug_hzb_ride_stall != 0 ? 1u : 0u);
    // tile / tilesX by multiplication: exact while (magic * tilesX - 2^32) * tile < 2^32 (checked by the caller)
    s.tilesXMagic = (uint32_t)((1ull << 32) / s.tilesX + 1ull);
    // ---- the run-time part of the schedule (struct Balance): whole rounds of the static deal in front, a pool of chunks behind
    s.staticClaims = 0xFFFFFFFFu;
    if (in.balance != 0 && groups >= 16u && groups <= 8u * in.claim_words) {
        constexpr uint32_t cs = kChunkShift;
        const uint32_t round = groups << cs;
        const uint32_t want_pool = (uint32_t)((uint64_t)s.numTiles * (uint32_t)in.balance_pool_16ths / 16u);
        // Chunks of 16 tiles (one tile per wave of a workgroup) and nothing smaller by default: a claim blocks its wave for ~1 us, and
        // with chunks of 4 tiles a workgroup needs one every 0.5 us - measured, that LOSES 1.5 us at 1080p and 2.2 us on a 540-row
        // band of a 4K frame (profiles/r04_balance.txt). A launch too short for `lookahead + 2` such chunks per workgroup is dealt
        // statically as a whole. (UR_OPT_BALANCE_CHUNK_SHIFT below 4 exists for the tests, which drive the claim path hard with it.)
        do {
            const uint32_t sh = (uint32_t)in.balance_chunk_shift;
            const uint32_t la = sh >= 4u ? 2u : (sh == 3u ? 3u : 4u); // chunks claimed ahead of use
            const uint32_t rounds = (s.numTiles - want_pool) / round;
            if ((rounds << cs) < 2u * WPB) break; // (the two tiles of a wave's prologue are static claims)
            const uint32_t static_tiles = rounds * round, chunks = (s.numTiles - static_tiles + (1u << sh) - 1u) >> sh;
            if (chunks < (la + 2u) * groups) break;
            if ((uint64_t)chunks * 8u / groups + la + 8u > kDynSlots) break; // a workgroup's slot table would not hold its word's share
            const unsigned long long magic = (((unsigned long long)chunks << 32) + groups - 1u) / groups;
            bool ok = true;
            for (uint32_t q8 = 0; q8 < groups && ok; q8 += 8u) {
                const uint32_t nq = std::min(8u, groups - q8);
                const uint32_t P0 = (uint32_t)((q8 * magic) >> 32), P1 = (uint32_t)(((q8 + nq) * magic) >> 32);
                ok = P1 >= P0 + la * nq && P1 <= chunks;
            }
            if (!ok) break;
            s.staticClaims = rounds << cs;
            s.poolChunks = chunks; s.staticTiles = static_tiles; s.dynShift = sh; s.lookahead = la;
            s.poolMagic = magic;
        } while (false);
    }
    const uint32_t sched[8] = {groups, s.numTiles, s.poolChunks != 0u ? s.staticTiles : s.numTiles, s.poolChunks, s.dynShift, s.lookahead, WPB, s.ride_pieces};
    std::copy(sched, sched + 8, s.reported);
    return s;
}

} // namespace ur
