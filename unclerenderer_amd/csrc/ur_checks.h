// The host-only view of the internals: what host callers outside the C-ABI units (the frame units, csrc/frame/) need of them. No device code
// and nothing of ur_ctx's layout: a plain C++ compiler takes it. ur_internal.h includes it; the definitions stay where they were
// (ur_api.hip, cull_api.hip, raster.hip, gbuffer_api.hip). Not installed.
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/ur_hotpath.h"
#include "../../include/ur_raster.h"

namespace ur {

void set_error(const char* fmt, ...);

// Do the byte ranges [a, a + a_bytes) and [b, b + b_bytes) share a byte?
inline bool overlaps(const void* a, size_t a_bytes, const void* b, size_t b_bytes)
{
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + b_bytes && y < x + a_bytes;
}
// Are rows [row0, row0 + rows) inside a w x h frame that is not empty? (rows == 0 is inside: an entry point that refuses an empty band
// says so beside the call.) The refusal's text stays the entry point's own.
inline bool band_in_frame(uint32_t w, uint32_t h, uint32_t row0, uint32_t rows) { return w != 0 && h != 0 && (uint64_t)row0 + rows <= h; }
// The Lighting, Sky and GpuDebugPrint entry points' check of the context, the frame and the band, with their text
inline int check_band(const char* who, const ur_ctx* ctx, uint32_t w, uint32_t h, uint32_t row0, uint32_t rows)
{
    if (!ctx || w == 0 || h == 0 || (uint64_t)row0 + rows > h) {
        set_error("%s: bad frame/band (w=%u h=%u row0=%u rows=%u)", who, w, h, row0, rows);
        return UR_EINVAL;
    }
    return UR_OK;
}

// ur_cull_indirect_args_views' checks of views that need no command count (ur_frame_set_cull_views)
int check_cull_views(const ur_cull_view* views, uint32_t view_count);
// The raster passes: one set of checks for the direct calls and the frame's setters; `who`, the entry point called, goes into the error text.
// Where the command slots live: the ranges' commands if ranges are set, else the draws' own
inline const void* raster_commands(const ur_raster_draws& draws) { return draws.ranges ? draws.ranges->commands : draws.commands; }
// (raster.hip) `target` not null; a list has both pointers; no list beside ranges; ranges whole; commands (unless command_count == 0) 16-byte, the rest 4-byte aligned
int check_raster_draws(const char* who, const ur_raster_draws& draws, const void* target, const char* target_name, const void* stats);
// ... behind what a direct call adds: the context, the matrices (ShadowMap passes its one twice), draws, w and h
int check_raster_call(const char* who, const ur_ctx* ctx, const float* m0, const float* m1, const ur_raster_draws* draws, const void* target, const char* target_name,
                      uint32_t w, uint32_t h, const void* stats);
inline int check_depth_flags(const char* who, uint32_t flags)
{
    if (flags & ~UR_DEPTH_QUANTIZE_D24) { set_error("%s: unknown flag bits 0x%x", who, flags & ~UR_DEPTH_QUANTIZE_D24); return UR_EINVAL; }
    return UR_OK;
}
int check_gbuffer_targets(const char* who, const ur_gbuffer_targets* targets); // (gbuffer_api.hip) none null but object_id; gbuf_a, gbuf_b, hdr 8-byte aligned, the others 4
// (gbuffer_api.hip) what ur_gbuffer_pass_masked adds: the masked draws' own checks, one key space, keys64, no overlap, no ObjectId
int check_gbuffer_mask(const char* who, const ur_raster_draws& draws, const ur_gbuffer_mask& mask, const ur_gbuffer_targets& targets, const float* depth, uint32_t w,
                       uint32_t h, uint32_t rows);
inline int check_key_triangle_bits(const char* who, uint32_t bits)
{
    if (bits > 31u) { set_error("%s: key_triangle_bits %u (0 = automatic, 1..31)", who, bits); return UR_EINVAL; }
    return UR_OK;
}
// T, the key's triangle bits, of a call over command_count slots: key_triangle_bits (checked above), or 32 - bit_length(command_count) when
// that is 0. UR_EUNSUPPORTED when the automatic split leaves fewer than 8 bits, UR_EINVAL when the slots do not fit beside the bits asked for
inline int split_key_bits(const char* who, uint32_t command_count, uint32_t key_triangle_bits, uint32_t& key_bits)
{
    key_bits = key_triangle_bits;
    if (key_bits == 0u) {
        if (command_count >= (1u << 24)) {
            set_error("%s: %u command slots leave fewer than 8 key bits for the triangle: pass key_triangle_bits", who, command_count);
            return UR_EUNSUPPORTED;
        }
        uint32_t length = 0u;
        while ((command_count >> length) != 0u) ++length;
        key_bits = 32u - length < 31u ? 32u - length : 31u;
    } else if ((uint64_t)command_count >= (1ull << (32u - key_bits))) {
        set_error("%s: %u command slots do not fit the %u key bits beside key_triangle_bits %u", who, command_count, 32u - key_bits, key_bits);
        return UR_EINVAL;
    }
    return UR_OK;
}

} // namespace ur
