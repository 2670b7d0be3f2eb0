// The C ABI of the ObjectId pass and the pick (include/ur_raster.h), host code only: the entry points, their
// argument checks, the raster launches (csrc/raster.hip, csrc/raster_pick.hip) and the arguments of the ObjectId resolve (csrc/gbuffer_resolve.hip). Built with
// the kernels' flags.

#include "gbuffer_resolve.h"
#include "raster_rule.h"
#include "ur_internal.h"

namespace {

using ur_raster::aligned;

// What both calls check alike: the context, the matrices, the draws, depth, the target's size, the flags and the key's split
int check_object_id_call(const char* who, const ur_ctx* ctx, const float* view, const float* projection, const ur_raster_draws* draws, const float* depth, uint32_t w,
                         uint32_t h, uint32_t flags, uint32_t key_triangle_bits, const void* stats6, uint32_t& key_bits)
{
    int rc = ur::check_raster_call(who, ctx, view, projection, draws, depth, "depth", w, h, stats6);
    if (rc == UR_OK) rc = ur::check_depth_flags(who, flags);
    if (rc == UR_OK) rc = ur::check_key_triangle_bits(who, key_triangle_bits);
    if (rc == UR_OK) rc = ur::split_key_bits(who, draws->command_count, key_triangle_bits, key_bits);
    return rc;
}

// Does [at, at + bytes) share a byte with depth (w x h floats) or the command slots?
bool overlaps_inputs(const void* at, size_t bytes, const ur_raster_draws& draws, const float* depth, uint32_t w, uint32_t h)
{
    const void* commands = ur::raster_commands(draws);
    return ur::overlaps(at, bytes, depth, (size_t)w * h * 4u) ||
           (commands && draws.command_count != 0u && ur::overlaps(at, bytes, commands, (size_t)draws.command_count * UR_INDIRECT_COMMAND_STRIDE));
}

} // namespace

extern "C" {

int ur_object_id_pass(ur_ctx* ctx, const float* view, const float* projection, const ur_raster_draws* draws, const float* depth, uint32_t* object_id, uint32_t* keys,
                      uint32_t w, uint32_t h, uint32_t row0, uint32_t rows, uint32_t flags, uint32_t key_triangle_bits, uint32_t* stats6)
{
    const char* who = "ur_object_id_pass";
    uint32_t key_bits = 0u;
    const int rc = check_object_id_call(who, ctx, view, projection, draws, depth, w, h, flags, key_triangle_bits, stats6, key_bits);
    if (rc != UR_OK) return rc;
    if (!object_id || !keys || !aligned(object_id, 4) || !aligned(keys, 4)) { ur::set_error("%s: a null or misaligned object_id or keys (4 bytes)", who); return UR_EINVAL; }
    if (rows == 0u || (uint64_t)row0 + rows > h) { ur::set_error("%s: rows [%u, %u + %u) of a target %u high", who, row0, row0, rows, h); return UR_EINVAL; }
    const size_t bytes = (size_t)w * rows * 4u;
    if (overlaps_inputs(object_id, bytes, *draws, depth, w, h) || overlaps_inputs(keys, bytes, *draws, depth, w, h) || ur::overlaps(object_id, bytes, keys, bytes)) {
        ur::set_error("%s: object_id or keys overlaps depth, the commands or the other target", who);
        return UR_EINVAL;
    }
    const int launched = ur::launch_visibility_raster(ctx, view, projection, draws, depth, keys, w, h, row0, rows, key_bits, (flags & UR_DEPTH_QUANTIZE_D24) != 0u, stats6);
    if (launched != UR_OK) return launched;
    ur::ObjectIdParams r{};
    r.commands = static_cast<const uint8_t*>(ur::raster_commands(*draws));
    r.mode = draws->visible_idx != nullptr ? 1u : 0u;
    r.visible_idx = draws->visible_idx; r.index_base = draws->index_base;
    r.keys = keys;
    r.n = w * rows; r.key_bits = key_bits;
    r.object_id = object_id;
    return ur::launch_object_id_resolve(ctx, r);
}

int ur_object_id_pick(ur_ctx* ctx, const float* view, const float* projection, const ur_raster_draws* draws, const float* depth, uint32_t w, uint32_t h, uint32_t flags,
                      uint32_t key_triangle_bits, const uint32_t* points_xy, uint32_t point_count, ur_pick_result* results, uint32_t* stats6)
{
    const char* who = "ur_object_id_pick";
    uint32_t key_bits = 0u;
    const int rc = check_object_id_call(who, ctx, view, projection, draws, depth, w, h, flags, key_triangle_bits, stats6, key_bits);
    if (rc != UR_OK) return rc;
    if (point_count > UR_PICK_MAX_POINTS) { ur::set_error("%s: %u points (at most %u)", who, point_count, UR_PICK_MAX_POINTS); return UR_EINVAL; }
    if (point_count == 0u) return UR_OK;
    if (!points_xy) { ur::set_error("%s: null points_xy with %u points", who, point_count); return UR_EINVAL; }
    if (!results || !aligned(results, 16)) { ur::set_error("%s: a null or misaligned results (16 bytes)", who); return UR_EINVAL; }
    if (overlaps_inputs(results, (size_t)point_count * sizeof(ur_pick_result), *draws, depth, w, h)) {
        ur::set_error("%s: results overlaps depth or the commands", who);
        return UR_EINVAL;
    }
    uint32_t points[UR_PICK_MAX_POINTS];
    for (uint32_t i = 0; i < point_count; ++i) { // the reference's clamp; w, h <= 16384: a coordinate fits 16 bits
        const uint32_t x = points_xy[2u * i] < w - 1u ? points_xy[2u * i] : w - 1u, y = points_xy[2u * i + 1u] < h - 1u ? points_xy[2u * i + 1u] : h - 1u;
        points[i] = x | (y << 16);
    }
    return ur::launch_object_id_pick(ctx, view, projection, draws, depth, w, h, key_bits, (flags & UR_DEPTH_QUANTIZE_D24) != 0u, points, point_count, results, stats6);
}

} // extern "C"
