// The Build HZB chain's layout, validity and steps (hzb_plan.h): integer arithmetic on plain values.
#include "hzb_plan.h"

#include <algorithm>

namespace ur {

uint32_t hzb_layout(uint32_t src_w, uint32_t src_h, ur_mip_desc* mips, uint32_t* mip_count)
{
    uint32_t w = (src_w + 1) / 2, h = (src_h + 1) / 2;
    w = w ? w : 1; h = h ? h : 1;
    uint32_t n = 0, off = 0;
    for (;;) {
        if (n >= UR_MAX_HZB_MIPS) return 0;
        mips[n].offset = off; mips[n].width = w; mips[n].height = h;
        ++n;
        off += (w * h + 63u) & ~63u; // every mip starts on a 256-byte boundary
        if (!(w > 1 || h > 1)) break;
        w = w / 2 ? w / 2 : 1; h = h / 2 ? h / 2 : 1;
    }
    *mip_count = n;
    return off;
}

bool valid_hzb_chain(uint32_t src_w, uint32_t src_h, const ur_mip_desc* mips, uint32_t mip_count)
{
    if (!mips || mip_count == 0 || mip_count > UR_MAX_HZB_MIPS) return false;
    uint32_t w = (src_w + 1) / 2, h = (src_h + 1) / 2;
    w = w ? w : 1; h = h ? h : 1;
    for (uint32_t m = 0; m < mip_count; ++m) {
        if (mips[m].width != w || mips[m].height != h) return false;
        w = w / 2 ? w / 2 : 1; h = h / 2 ? h / 2 : 1;
    }
    return true;
}

bool valid_hzb_chain_below_mip0(const ur_mip_desc* mips, uint32_t mip_count)
{
    if (!mips || mip_count == 0 || mip_count > UR_MAX_HZB_MIPS) return false;
    uint32_t w = mips[0].width, h = mips[0].height;
    if (w == 0 || h == 0) return false;
    uint64_t end = 0;
    for (uint32_t m = 0; m < mip_count; ++m) {
        if (mips[m].width != w || mips[m].height != h) return false;
        if (m != 0 && mips[m].offset < end) return false;
        end = (uint64_t)mips[m].offset + (uint64_t)w * h;
        w = w / 2 ? w / 2 : 1; h = h / 2 ? h / 2 : 1;
    }
    return true;
}

void hzb_band_pieces(uint32_t src_h, uint32_t n_ranks, uint32_t rank, uint32_t* piece_row0, uint32_t* piece_rows)
{
    const uint32_t rows = src_h / n_ranks;
    const uint32_t first = (rank * rows + 31u) / 32u, last = ((rank + 1u) * rows + 31u) / 32u; // pieces whose first source row lies in the band
    *piece_row0 = first;
    *piece_rows = last - first;
}

void hzb_band_slices(const ur_mip_desc* mips, uint32_t piece_row0, uint32_t piece_rows, ur_hzb_slice* out5)
{
    for (uint32_t k = 0; k < 5; ++k) {
        const uint32_t per = 16u >> k, H = mips[k].height, W = mips[k].width;
        const uint32_t r0 = std::min(piece_row0 * per, H), r1 = std::min((piece_row0 + piece_rows) * per, H);
        out5[k].offset = mips[k].offset + r0 * W;
        out5[k].count = (r1 - r0) * W;
    }
}

namespace {

// Can the single-workgroup tail take the chain from level `mip` on?
bool tail_can_start(const ur_mip_desc* mips, uint32_t mip_count, uint32_t mip)
{
    return mip_count > mip && (uint64_t)mips[mip].width * mips[mip].height <= kTailTexels && mip_count - mip <= kTailMaxLevels;
}

// Levels of the wide step that starts at `mip`. Same grouping as the reference's while-loop (DeferredRenderer.cpp:1046-1207): <=4 mips
// per launch ...
uint32_t wide_levels(const ur_mip_desc* mips, uint32_t mip_count, uint32_t mip)
{
    uint32_t n = (mip_count - mip) < 4u ? (mip_count - mip) : 4u;
    // the first launch also produces mip 4 when a tail launch follows: the tail then starts from 1/4 of the texels
    // (a single workgroup reads ~25 GB/s: 130 KB of mip 3 at 4K would be 5 us on its own)
    if (mip == 0 && mip_count > 4u && (uint64_t)mips[4].width * mips[4].height <= kTailTexels) n = 5u;
    // What has to fit the tail's LDS is ITS first level, mip 5; its parent, mip 4, is read from global memory: at 8K 130 KB
    // through one workgroup. With 4-byte taps that was a 9-us tail (slower than a third launch); with the 16-byte loads of
    // tail_first_level_vec it is two launches for every chain up to 8K.
    else if (mip == 0 && tail_can_start(mips, mip_count, 5u)) n = 5u;
    return n;
}

HzbStep wide_step(const ur_mip_desc* mips, uint32_t first, uint32_t levels, bool hold)
{
    HzbStep s{};
    s.kind = HzbStep::wide;
    s.from_depth = first == 0;
    s.hold = hold;
    s.first = first; s.levels = levels;
    s.grid_x = (mips[first].width + 63u) / 64u;
    s.grid_y = (mips[first].height + 15u) / 16u;
    return s;
}

HzbStep tail_step(uint32_t mip_count, uint32_t first, bool hold)
{
    HzbStep s{};
    s.kind = HzbStep::tail;
    s.hold = hold;
    s.first = first; s.levels = mip_count - first;
    return s;
}

void push(HzbPlan& p, const HzbStep& s)
{
    if (p.count < kMaxHzbSteps) p.steps[p.count++] = s;
}

} // namespace

bool hzb_chain_is_wide_plus_tail(const ur_mip_desc* mips, uint32_t mip_count) { return tail_can_start(mips, mip_count, 5u); }

HzbPlan plan_hzb_chain(uint32_t src_w, uint32_t src_h, const ur_mip_desc* mips, uint32_t mip_count, int mode, bool can_hold_wide)
{
    HzbPlan p{};
    if (src_w == 0 || src_h == 0 || !valid_hzb_chain(src_w, src_h, mips, mip_count)) { p.status = HzbPlan::invalid_chain; return p; }
    // ... first launch reads the depth buffer with clamped 2x2 footprints, later launches read the last mip of the previous launch —
    // until the remaining levels fit one workgroup's LDS: those run in a single launch with the same values.
    uint32_t mip = 0;
    while (mip < mip_count) {
        if (mip > 0 && tail_can_start(mips, mip_count, mip)) {
            // mode 1, 2: the next streaming Lighting launch takes it along (lighting.hip, planned in lighting_plan.cpp); ur_flush otherwise
            push(p, tail_step(mip_count, mip, mode != 0));
            break;
        }
        const uint32_t n = wide_levels(mips, mip_count, mip);
        // ur_defer_hzb_tail(ctx, 2): a chain that is ONE five-level launch from the depth buffer plus the single-workgroup tail
        // (1080p, 4K and 8K all are) is held back as a whole: the next streaming Lighting launch takes its 128x32 pieces
        // along (lighting.hip, if lighting_plan.cpp finds that they can ride), ur_flush / a cull / another build launch it the ordinary way
        const bool hold = mip == 0 && n == 5u && mode == 2 && can_hold_wide && hzb_chain_is_wide_plus_tail(mips, mip_count);
        push(p, wide_step(mips, mip, n, hold));
        mip += n;
    }
    return p;
}

// ---- band-sharded chain (multi-GPU, SURVEY.md section 8e row 3's alternative): a rank builds mips 0..4 for the 128x32 source pieces
// whose first row lies in its band - every value of those levels depends on its own piece only, so the slices are the whole-frame
// launch's bits -, the slices are all-gathered by the host, and the single-workgroup tail (mips 5..) runs on every rank behind it.
HzbPlan plan_hzb_band(uint32_t src_w, uint32_t src_h, const ur_mip_desc* mips, uint32_t mip_count, int mode, uint32_t piece_row0, uint32_t piece_rows)
{
    HzbPlan p{};
    if (src_w == 0 || src_h == 0 || !valid_hzb_chain(src_w, src_h, mips, mip_count)) { p.status = HzbPlan::invalid_chain; return p; }
    if (!hzb_chain_is_wide_plus_tail(mips, mip_count)) { p.status = HzbPlan::not_wide_plus_tail; return p; }
    if (piece_rows == 0u) return p;
    HzbStep s = wide_step(mips, 0u, 5u, mode == 2); // mode 2: rides the next streaming Lighting launch (no tail: it waits for the gather)
    s.grid_y = piece_rows;
    s.by0 = piece_row0;
    push(p, s);
    return p;
}

HzbPlan plan_hzb_tail(const ur_mip_desc* mips, uint32_t mip_count)
{
    HzbPlan p{};
    if (!valid_hzb_chain_below_mip0(mips, mip_count)) { p.status = HzbPlan::invalid_chain; return p; }
    if (!hzb_chain_is_wide_plus_tail(mips, mip_count)) { p.status = HzbPlan::not_wide_plus_tail; return p; }
    push(p, tail_step(mip_count, 5u, false));
    return p;
}

} // namespace ur
