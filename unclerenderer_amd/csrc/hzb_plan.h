// Host decisions of Build HZB that need no device: the mip chain's layout and validity, a band's share of it, and the steps one chain
// takes (which levels each launch produces, from what, on which grid, and whether it goes out now or is held back for the next
// streaming Lighting launch). Plain C++17 (no HIP header, no ur_ctx), so a test drives it without a GPU (tests/cpp/test_hzb_plan.cpp).
// A plan holds offsets and sizes only, never pointers: csrc/hzb.hip binds its steps to buffers and launches or holds them. Not installed.
#pragma once

#include <cstdint>

#include "../../include/ur_hotpath.h"

namespace ur {

// The single-workgroup tail of the chain (csrc/hzb_tail.h) takes the levels from its first on: at most kTailMaxLevels of them, the first
// of at most kTailTexels texels (its two level buffers are LDS).
constexpr uint32_t kTailMaxLevels = 12, kTailTexels = 16384;

// ---- the chain's layout (ur_hzb_layout, ur_hzb_band_pieces, ur_hzb_band_slices: the entry points add the argument checks and error texts)
// total floats, 0 when the chain would need more than UR_MAX_HZB_MIPS levels; mips: UR_MAX_HZB_MIPS entries
uint32_t hzb_layout(uint32_t src_w, uint32_t src_h, ur_mip_desc* mips, uint32_t* mip_count);
// the chain ur_hzb_layout gives a src_w x src_h depth buffer: sizes only (CreateHZBResources), the offsets are the caller's
bool valid_hzb_chain(uint32_t src_w, uint32_t src_h, const ur_mip_desc* mips, uint32_t mip_count);
// the levels below mips[0] halve by FLOOR (CreateHZBResources, DeferredRenderer.cpp:2801-2835); every level lies inside the
// allocation the layout describes (offsets ascending, no overlap)
bool valid_hzb_chain_below_mip0(const ur_mip_desc* mips, uint32_t mip_count);
// the 128x32 source pieces whose first row lies in rank's band of src_h / n_ranks rows (src_h a multiple of n_ranks, rank < n_ranks)
void hzb_band_pieces(uint32_t src_h, uint32_t n_ranks, uint32_t rank, uint32_t* piece_row0, uint32_t* piece_rows);
// what those pieces write of mips 0..4 (mip_count >= 5)
void hzb_band_slices(const ur_mip_desc* mips, uint32_t piece_row0, uint32_t piece_rows, ur_hzb_slice* out5);

// ---- the steps of one chain --------------------------------------------------------------------------------------------------------------
struct HzbStep {
    enum Kind : uint8_t { wide, tail } kind;
    bool from_depth;          // wide: reads the depth buffer (the chain's first step only); otherwise mip first - 1, as a tail always does
    bool hold;                // not launched now: kept on the context for the next streaming Lighting launch (ur_defer_hzb_tail), or ur_flush
    uint32_t first, levels;   // produces mips [first, first + levels)
    uint32_t grid_x, grid_y;  // wide: workgroups, one per 128x32 source piece ...
    uint32_t by0;             // ... the first piece row (0 but for a band's share: ur_build_hzb_band)
};

constexpr uint32_t kMaxHzbSteps = 5; // (every wide step but the last takes four levels or five)

struct HzbPlan {
    enum Status : uint8_t { ok, invalid_chain, not_wide_plus_tail } status;
    uint32_t count;
    HzbStep steps[kMaxHzbSteps]; // in launch order; at most one tail, the last
};

// "One five-level launch from the depth buffer plus the single-workgroup tail" (1080p, 4K and 8K all are): the only chain whose wide
// step can be held back, split into bands or left without its tail.
bool hzb_chain_is_wide_plus_tail(const ur_mip_desc* mips, uint32_t mip_count);

// ur_build_hzb. mode: ur_defer_hzb_tail's (0 off, 1 the tail is held, 2 the whole chain is when it is wide plus tail and the context
// `can_hold_wide`: it owns the arrival counter the riding tail waits on). invalid_chain: mips is not valid_hzb_chain of the source.
HzbPlan plan_hzb_chain(uint32_t src_w, uint32_t src_h, const ur_mip_desc* mips, uint32_t mip_count, int mode, bool can_hold_wide = true);
// ur_build_hzb_band: the wide step alone, piece_rows rows of pieces from piece_row0 (no step when there are none); held in mode 2
HzbPlan plan_hzb_band(uint32_t src_w, uint32_t src_h, const ur_mip_desc* mips, uint32_t mip_count, int mode, uint32_t piece_row0, uint32_t piece_rows);
// ur_build_hzb_tail: the tail alone, launched whatever the mode (invalid_chain: not valid_hzb_chain_below_mip0)
HzbPlan plan_hzb_tail(const ur_mip_desc* mips, uint32_t mip_count);

} // namespace ur
