// What the host hands the kernels of the raster passes and the pick (csrc/raster.hip, csrc/raster_mask.hip, csrc/raster_pick.hip): the
// parameter blocks, the snapped triangle, the large queue's layout, and the one function that fills what every launch shares, the split of
// the work into (candidate, segment) items included.
#pragma once

#include "raster_rule.h"
#include "ur_internal.h"

namespace {

using namespace ur_raster;

constexpr uint32_t kQueueHeaderDwords = 16u; // the count on a line of its own
constexpr uint32_t kEntryDwords = 12u;       // x0 y0 x1 y1 | x2 y2 z0 k1 | k2 tile box_min box_max
constexpr uint32_t kKeyedEntryDwords = 16u;  // GBuffer: | key - - - behind them; the queue is allocated for entries of this size
constexpr uint32_t kLargeStamps = 64u;       // a bounding box of more 8 x 8 stamps than this is a large triangle
constexpr uint32_t kOwnPixels = 4u;          // a bounding box of at most this many centres is rasterised by the triangle's own lane
constexpr uint32_t kNoTile = 0xFFFFFFFFu;

struct RasterParams {
    const uint8_t* commands;
    uint32_t command_count;
    uint32_t mode; // 0 every slot, 1 list, 2 ranges
    const uint32_t* visible_idx;
    const uint32_t* visible_count;
    uint32_t index_base;
    uint32_t range_count;
    const uint32_t* offsets;
    const uint32_t* counts;
    float L[16];  // ShadowMap: LightViewProjection; DepthPrepass: View
    float Pr[16]; // DepthPrepass: Projection
    uint32_t* map;
    uint32_t w, h;
    float half_w, half_h; // 0.5f * w, 0.5f * h
    uint32_t* stats;
    uint32_t* queue; // 64-bit count at [0..1], entries from kQueueHeaderDwords; null without room
    uint32_t queue_cap;
    uint32_t segments, items; // items = candidates * segments
    // GBuffer: `map` is the key image of the band [row0, row0 + rows); depth is the whole target, read only
    const float* depth;
    uint32_t row0, rows, key_bits;
};

// What the masked policy's kernels take behind a RasterParams: `map` is then the band's 64-bit words
struct MaskArgs {
    const ur_material* materials; // null: no slot has a material (nothing is discarded)
    uint32_t material_count;
    const float* lod; // 127 thresholds of the level of detail
};
struct MaskedParams : RasterParams {
    MaskArgs mask;
};

// What the pick kernels take behind a RasterParams: `map`, the band and the queue are not used. The points ride in the
// kernel arguments, 256 bytes for the most there can be
struct PickParams : RasterParams {
    uint32_t point_count;
    uint32_t points[UR_PICK_MAX_POINTS]; // x | y << 16, clamped to the target
    unsigned long long* results;         // 16-byte records: the first 8 bytes of record i take (key << 32) | depth bits
};

struct Tri {
    int x0, y0, x1, y1, x2, y2; // 24.8 target space, y down
    float z0, k1, k2;
};

// What GBuffer's raster has beside a depth pass': the depth it tests against, its band and the key's triangle bits
struct VisArgs {
    const float* depth;
    uint32_t row0, rows, key_bits;
};

// What the raster and the pick launch alike: the selection, the matrices, the target's size, the counters, GBuffer's depth, band and key
// bits, and the split of the work into (candidate, segment) items - enough waves to fill the device whatever the command count, since
// index counts live on the device. Returns the blocks of the launch. command_count is not 0.
inline uint32_t fill_raster_params(RasterParams& p, const ur_ctx* ctx, const float* m0, const float* m1, const ur_raster_draws* draws, uint32_t w, uint32_t h,
                                   uint32_t* stats, const VisArgs* vis)
{
    const ur_draw_ranges* rg = draws->ranges;
    p.commands = static_cast<const uint8_t*>(ur::raster_commands(*draws));
    p.command_count = draws->command_count;
    p.mode = draws->visible_idx != nullptr ? 1u : (rg ? 2u : 0u);
    p.visible_idx = draws->visible_idx; p.visible_count = draws->visible_count; p.index_base = draws->index_base;
    if (rg) { p.range_count = rg->range_count; p.offsets = rg->offsets; p.counts = rg->counts; }
    for (int k = 0; k < 16; ++k) { p.L[k] = m0[k]; p.Pr[k] = m1 ? m1[k] : 0.0f; }
    p.w = w; p.h = h;
    p.half_w = 0.5f * (float)w; p.half_h = 0.5f * (float)h;
    p.stats = stats;
    if (vis) { p.depth = vis->depth; p.row0 = vis->row0; p.rows = vis->rows; p.key_bits = vis->key_bits; }
    const uint32_t want_waves = (uint32_t)ctx->cu_count * 16u;
    p.segments = max(1u, min(1024u, want_waves / p.command_count));
    const uint64_t items = (uint64_t)p.command_count * p.segments;
    p.items = (uint32_t)items;
    if (items > 0xFFFFFFFFull) { p.segments = 1u; p.items = p.command_count; }
    return min((p.items + kWaves - 1u) / kWaves, (uint32_t)ctx->cu_count * 32u);
}

} // namespace
