// Host decisions of a Lighting launch that need no device: the staged environment cube's layout and the schedule of a streaming
// launch. Plain C++17 (no HIP header, no ur_ctx), so a test drives it without a GPU (tests/cpp/test_lighting_plan.cpp). Not installed.
#pragma once

#include <cstdint>

struct ur_half4; // include/ur_hotpath.h

namespace ur {

constexpr uint32_t kChunkShift = 2;       // static deal: chunks of 4 consecutive tiles (4K, round 1: chunks of 16 / 4 / 1 tiles -> 75.4 / 74.6 / 79.1 us)
constexpr uint32_t kDynSlots = 256;       // run-time chunk slots of a streaming workgroup (csrc/lighting.hip, dyn_claim)
constexpr uint32_t kLdsCubeBytes = 32768; // a streaming workgroup's LDS copy of the cube's small mips: their RGB row-pair entries
                                          // (the shipped 256^2 cube: mips 4..8 = 31 968 bytes)

// ---- the staged environment cube (ur_stage_env_cube writes it, ur_env_cube_texels sizes it, both lighting kernels read it) -----------
// Two sections of 8-byte half4 units. First every mip as six bordered faces of edge E = max(1, base >> m) + 2 (border = the seamless
// neighbours). Behind all of them every mip once more as RGB ROW PAIRS: entry (f, j, i), j in [0, E - 2], is the 12 bytes {R G B of
// texel (i, j), R G B of texel (i, j + 1)} of the bordered face, 6 (E - 1) E entries per mip = 9 (E - 1) E half4 units.
struct CubeLayout {
    uint32_t mips;          // 0: refused (a zero base size, no mip or more than 16)
    uint64_t edge[16];      // E of mip m, computed in 32 bits as ur_env_cube_texels always has: base sizes of 2^32 - 2 and 2^32 - 1 wrap to
                            // E = 0 and 1 (sizes nobody can stage; the entry point's answers for them are kept). 64 bits wide for the products
    uint64_t bordered[16];  // where mip m's bordered faces start, in half4 texels
    uint64_t pairs[17];     // where mip m's row-pair entries start, in BYTES; [mips] = bytes
    uint64_t texels, bytes; // the whole buffer, in half4 texels and in bytes
    uint32_t size(uint32_t m) const { return (uint32_t)(edge[m] - 2u); } // max(1, base >> m)
};
CubeLayout cube_layout(uint32_t base_size, uint32_t mip_count);
// The first of the smallest mips whose row-pair entries together fit `budget` bytes (L.mips: not even the last one does)
uint32_t cube_first_mip_within(const CubeLayout& L, uint64_t budget);
// (env_cube_stage.cpp) Writes both sections into `out`, L.texels half4 units of host memory, from the source cube `src`: face-major, every
// face its mips 0 .. L.mips - 1 of size(m)^2 texels one after the other. ur_stage_env_cube copies the result to the device.
void stage_env_cube_host(const ur_half4* src, const CubeLayout& L, ur_half4* out);

// ---- the schedule of one streaming launch ------------------------------------------------------------------------------------------------
struct StreamPlanInput {
    int cus;           // ur_ctx::cu_count
    int leave_cus, ride_walkers, balance, balance_pool_16ths, balance_chunk_shift, debug_hzb_ride_stall; // ur_ctx::Options, as set
    uint32_t W, rows;  // the band: W a multiple of 16, at least 32
    uint32_t wpb;      // waves per workgroup: 16 or 12
    bool tail_pending; // a held-back HZB tail waits on the context (ur_defer_hzb_tail) ...
    bool wide_pending; // ... and the wide launch in front of it, or a band's share of it (ur_build_hzb_band), of this grid:
    uint32_t wide_grid_x, wide_grid_y;
    uint32_t claim_words; // claim words the context owns (0: none, no run-time part)
};

struct StreamPlan {
    uint32_t tilesX, numTiles, tilesXMagic; // tile / tilesX = (tile * tilesXMagic) >> 32
    uint32_t groups;                        // lighting workgroups
    bool carry_tail;                        // one more workgroup runs the pending tail (and the launch consumes it)
    bool rides;                             // the pending wide launch's pieces ride (the launch consumes them); beside a carried tail their walkers report to it
    uint32_t ride_pieces, ride_grid_x, ride_walkers, ride_want, ride_spin_limit;
    bool flush_first;                       // pieces are pending and cannot ride: the chain's ordinary launches go out in front
    uint32_t staticClaims;                  // StreamHot::staticClaims
    uint32_t poolChunks, staticTiles, dynShift, lookahead; // struct Balance (poolChunks 0: off)
    unsigned long long poolMagic;
    uint32_t reported[8];                   // ur_debug_lighting_schedule
};
StreamPlan plan_stream(const StreamPlanInput& in);

// Waves of a workgroup that walk riding HZB pieces. The chain should be done within about a quarter of the shading (a piece is ~3 us of
// one wave's time, a tile ~1.75 us): walkers >= 7 x pieces-per-workgroup / tiles-per-wave, rounded up to a power of two
// (UR_OPT_RIDE_WALKERS forces the count); then one of the kernel's two forms: the last wave alone, or all of them.
uint32_t ride_walkers(uint32_t pieces, uint32_t tiles, uint32_t lighting_groups, uint32_t wpb, int forced);

} // namespace ur
