// The C ABI of the GBuffer and the Forward pass (include/ur_raster.h; DESIGN.md sections 3.9 to 3.12), host code only: the entry points,
// their argument checks, the raster launches (csrc/raster.hip, csrc/raster_mask.hip) and the arguments of the two resolves (csrc/gbuffer_resolve.hip,
// csrc/forward_resolve.hip). The Forward pass' entry points share gbuffer_entry's checks and raster launches. Built with the kernels' flags.

#include "forward_resolve.h"
#include "gbuffer_resolve.h"
#include "lighting_plan.h"
#include "raster_rule.h"
#include "ur_internal.h"

namespace {

using ur_raster::aligned;

// What ur_forward_pass adds to a GBuffer call: its targets are hdr and keys alone, and the resolve shades (csrc/forward_resolve.hip)
struct ForwardCall {
    const ur_scene_constants* frame;
    const ur_lighting_tables* tables;
};

// ur_forward_pass' own checks (the draws, depth and the matrices have passed theirs); fills in the staged cube's layout
int check_forward_call(const char* who, const ForwardCall& f, const ur_gbuffer_targets* targets, const ur_raster_draws& draws, const float* depth,
                       const ur_material* materials, uint32_t material_count, uint32_t w, uint32_t h, uint32_t rows, ur::CubeLayout& cube)
{
    if (!targets || !targets->hdr || !targets->keys) { ur::set_error("%s: null targets, hdr or keys", who); return UR_EINVAL; }
    if (!aligned(targets->hdr, 8) || !aligned(targets->keys, 4)) { ur::set_error("%s: a misaligned target (hdr 8 bytes, keys 4)", who); return UR_EINVAL; }
    if (!f.frame || !f.tables) { ur::set_error("%s: null frame_constants or tables", who); return UR_EINVAL; }
    const ur_lighting_tables& t = *f.tables;
    const float sw = f.frame->ShadowMapSize[0], sh = f.frame->ShadowMapSize[1];
    const bool shadows = f.frame->ShadowStrength > 0.0f;
    if (shadows && (!t.shadow_map || !(sw >= 1.0f && sw <= (float)UR_RASTER_MAX_TARGET) || !(sh >= 1.0f && sh <= (float)UR_RASTER_MAX_TARGET))) {
        ur::set_error("%s: ShadowStrength > 0 without a shadow map, or a ShadowMapSize outside 1..%u", who, UR_RASTER_MAX_TARGET);
        return UR_EINVAL;
    }
    if (!t.env_cube || t.env_base_size == 0u || t.env_mip_count == 0u || t.env_mip_count > 16u || !t.brdf_lut_rg16 || t.lut_width == 0u || t.lut_height == 0u ||
        !aligned(t.env_cube, 8) || !aligned(t.brdf_lut_rg16, 4) || !aligned(t.shadow_map, 4)) {
        ur::set_error("%s: bad lighting tables (a null or misaligned cube or LUT, a zero size, no mip or more than 16)", who);
        return UR_EINVAL;
    }
    cube = ur::cube_layout(t.env_base_size, t.env_mip_count);
    if (cube.mips == 0u || t.env_cube_texels != cube.texels) {
        ur::set_error("%s: ur_lighting_tables.env_cube_texels = %llu, but ur_stage_env_cube writes %llu texels for a %u^2 cube of %u mips", who,
                      (unsigned long long)t.env_cube_texels, (unsigned long long)cube.texels, t.env_base_size, t.env_mip_count);
        return UR_EINVAL;
    }
    const size_t n = (size_t)w * rows;
    const struct { const void* at; size_t bytes; } inputs[] = {
        {depth, (size_t)w * h * 4u}, {ur::raster_commands(draws), (size_t)draws.command_count * UR_INDIRECT_COMMAND_STRIDE},
        {materials, (size_t)material_count * sizeof(ur_material)}, {shadows ? t.shadow_map : nullptr, (size_t)sw * (size_t)sh * 4u},
        {t.env_cube, (size_t)cube.texels * 8u}, {t.brdf_lut_rg16, (size_t)t.lut_width * t.lut_height * 4u}};
    for (const auto& in : inputs) {
        if (in.at && in.bytes && (ur::overlaps(targets->hdr, n * 8u, in.at, in.bytes) || ur::overlaps(targets->keys, n * 4u, in.at, in.bytes))) {
            ur::set_error("%s: hdr or keys overlaps an input (depth, the commands, the materials or a lighting table)", who);
            return UR_EINVAL;
        }
    }
    if (ur::overlaps(targets->hdr, n * 8u, targets->keys, n * 4u)) { ur::set_error("%s: hdr overlaps keys", who); return UR_EINVAL; }
    return UR_OK;
}

// What the arguments of the two resolves share: the commands and the selection, the matrices, the keys and their band, the key's split,
// the material table with the sampler's tables and, with `mask` (passed only under visible lists), the masked selection's list
void fill_key_params(ur::KeyParams& r, const ur_ctx* ctx, const float* view, const float* projection, const ur_raster_draws& draws, const uint32_t* keys, uint32_t w, uint32_t h,
                     uint32_t row0, uint32_t rows, uint32_t key_bits, const ur_material* materials, uint32_t material_count, const ur_gbuffer_mask* mask)
{
    r.commands = static_cast<const uint8_t*>(ur::raster_commands(draws));
    r.mode = draws.visible_idx != nullptr ? 1u : 0u;
    r.visible_idx = draws.visible_idx; r.index_base = draws.index_base;
    for (int k = 0; k < 16; ++k) { r.V[k] = view[k]; r.Pr[k] = projection[k]; }
    r.keys = keys;
    r.w = w; r.row0 = row0; r.n = w * rows;
    r.half_w = 0.5f * (float)w; r.half_h = 0.5f * (float)h;
    r.key_bits = key_bits;
    r.materials = materials; r.material_count = material_count;
    r.decode = ctx->srgb_table; r.lod = ctx->lod_table;
    if (mask) {
        r.keys64 = reinterpret_cast<const unsigned long long*>(mask->keys64);
        r.mask_mode = mask->draws->visible_idx != nullptr ? 1u : 0u;
        r.mask_visible_idx = mask->draws->visible_idx; r.mask_index_base = mask->draws->index_base;
    }
}

// The checks and the launches behind the GBuffer and the Forward entry points; `who` names the caller in the error text, `who_parts` its
// _parts form; `forward`: ur_forward_pass (targets then holds hdr and keys alone)
int gbuffer_entry(const char* who, const char* who_parts, ur_ctx* ctx, const float* view, const float* projection, const ur_raster_draws* draws, const float* depth,
                  const ur_gbuffer_targets* targets, uint32_t w, uint32_t h, uint32_t row0, uint32_t rows, uint32_t flags, uint32_t key_triangle_bits,
                  uint32_t* stats6, uint32_t parts, const ur_material* materials, uint32_t material_count, const ur_gbuffer_mask* mask = nullptr,
                  float* depth_out = nullptr, const ForwardCall* forward = nullptr)
{
    ur::CubeLayout cube{};
    int rc = ur::check_raster_call(who, ctx, view, projection, draws, depth, "depth", w, h, stats6);
    if (rc == UR_OK) rc = ur::check_depth_flags(who, flags);
    if (rc == UR_OK && !forward) rc = ur::check_gbuffer_targets(who, targets);
    if (rc == UR_OK) rc = ur::check_key_triangle_bits(who, key_triangle_bits);
    if (rc != UR_OK) return rc;
    if (rows == 0u || (uint64_t)row0 + rows > h) { ur::set_error("%s: rows [%u, %u + %u) of a target %u high", who, row0, row0, rows, h); return UR_EINVAL; }
    if (parts == 0u || (parts & ~(UR_GBUFFER_PART_RASTER | UR_GBUFFER_PART_RESOLVE))) { ur::set_error("%s: parts 0x%x (UR_GBUFFER_PART_RASTER | UR_GBUFFER_PART_RESOLVE)", who_parts, parts); return UR_EINVAL; }
    uint32_t key_bits = 0u;
    rc = ur::split_key_bits(who, draws->command_count, key_triangle_bits, key_bits);
    if (rc != UR_OK) return rc;
    if (!aligned(materials, 16)) { ur::set_error("%s: a misaligned material table (16 bytes)", who); return UR_EINVAL; }
    if (forward) {
        rc = check_forward_call(who, *forward, targets, *draws, depth, materials, material_count, w, h, rows, cube);
        if (rc != UR_OK) return rc;
    }
    if (mask) {
        rc = ur::check_gbuffer_mask(who, *draws, *mask, *targets, depth, w, h, rows);
        if (rc != UR_OK) return rc;
    }
    // ---- the launches: the raster over the key image (UR_GBUFFER_PART_RASTER), then the resolve (UR_GBUFFER_PART_RESOLVE)
    if (parts & UR_GBUFFER_PART_RASTER) {
        rc = ur::launch_visibility_raster(ctx, view, projection, draws, depth, targets->keys, w, h, row0, rows, key_bits, (flags & UR_DEPTH_QUANTIZE_D24) != 0u, stats6);
        if (rc != UR_OK) return rc;
        if (mask) {
            rc = ur::launch_masked_raster(ctx, view, projection, mask->draws, depth_out, mask->keys64, targets->keys, w, h, row0, rows, key_bits,
                                          (flags & UR_DEPTH_QUANTIZE_D24) != 0u, mask->stats6, materials, material_count, mask->won);
            if (rc != UR_OK) return rc;
        }
    }
    if (!(parts & UR_GBUFFER_PART_RESOLVE)) return UR_OK;
    const bool lists = mask && (draws->visible_idx != nullptr || mask->draws->visible_idx != nullptr);
    if (forward) {
        ur::ForwardParams f{};
        fill_key_params(f, ctx, view, projection, *draws, targets->keys, w, h, row0, rows, key_bits, materials, material_count, lists ? mask : nullptr);
        f.hdr = reinterpret_cast<uint2*>(targets->hdr);
        const ur_scene_constants& S = *forward->frame;
        const ur_lighting_tables& T = *forward->tables;
        for (int k = 0; k < 16; ++k) f.lvp[k] = S.LightViewProjection[k];
        for (int k = 0; k < 3; ++k) { f.camera[k] = S.CameraPosition[k]; f.light_direction[k] = S.LightDirection[k]; f.light_color[k] = S.LightColor[k]; }
        f.light_intensity = S.LightIntensity;
        f.shadow_strength = S.ShadowStrength; f.shadow_bias = S.ShadowBias;
        f.shadow_size[0] = S.ShadowMapSize[0]; f.shadow_size[1] = S.ShadowMapSize[1];
        const float above = S.EnvMapMipCount - 1.0f;
        f.max_mip = above > 0.0f ? above : 0.0f;
        f.shadow = T.shadow_map;
        f.shadow_w = S.ShadowStrength > 0.0f ? (int)S.ShadowMapSize[0] : 0; f.shadow_h = S.ShadowStrength > 0.0f ? (int)S.ShadowMapSize[1] : 0;
        f.env = reinterpret_cast<const uint2*>(T.env_cube);
        f.env_base = T.env_base_size; f.env_mips = T.env_mip_count;
        for (uint32_t m = 0; m < 16u; ++m) f.env_offset[m] = m < T.env_mip_count ? (uint32_t)cube.bordered[m] : 0u;
        f.lut = reinterpret_cast<const uint32_t*>(T.brdf_lut_rg16);
        f.lut_w = T.lut_width; f.lut_h = T.lut_height;
        return ur::launch_forward_resolve(ctx, f, materials != nullptr, lists);
    }
    ur::ResolveParams r{};
    fill_key_params(r, ctx, view, projection, *draws, targets->keys, w, h, row0, rows, key_bits, materials, material_count, lists ? mask : nullptr);
    r.gbuf_a = reinterpret_cast<uint2*>(targets->gbuf_a); r.gbuf_b = reinterpret_cast<uint2*>(targets->gbuf_b); r.gbuf_c = targets->gbuf_c;
    r.hdr = reinterpret_cast<uint2*>(targets->hdr); r.object_id = targets->object_id;
    r.table = ctx->srgb_encode_table;
    // (an ordinal is a position in its own selection's list: under lists the resolve looks at keys64; no ObjectId beside a mask)
    return ur::launch_gbuffer_resolve(ctx, r, targets->object_id != nullptr, materials != nullptr, lists);
}

} // namespace

int ur::check_gbuffer_targets(const char* who, const ur_gbuffer_targets* targets)
{
    if (!targets || !targets->gbuf_a || !targets->gbuf_b || !targets->gbuf_c || !targets->hdr || !targets->keys) {
        ur::set_error("%s: null targets, or a null target other than object_id", who);
        return UR_EINVAL;
    }
    if (!aligned(targets->gbuf_a, 8) || !aligned(targets->gbuf_b, 8) || !aligned(targets->hdr, 8) || !aligned(targets->gbuf_c, 4) || !aligned(targets->object_id, 4) ||
        !aligned(targets->keys, 4)) {
        ur::set_error("%s: a misaligned target (gbuf_a, gbuf_b, hdr 8 bytes, the others 4)", who);
        return UR_EINVAL;
    }
    return UR_OK;
}

// The checks ur_gbuffer_pass_masked adds; the opaque draws, the targets and depth have passed theirs
int ur::check_gbuffer_mask(const char* who, const ur_raster_draws& draws, const ur_gbuffer_mask& mask, const ur_gbuffer_targets& targets, const float* depth, uint32_t w,
                           uint32_t h, uint32_t rows)
{
    if (!mask.draws) { set_error("%s: a mask without draws", who); return UR_EINVAL; }
    const int rc = check_raster_draws(who, *mask.draws, depth, "depth", mask.stats6);
    if (rc != UR_OK) return rc;
    if (raster_commands(*mask.draws) != raster_commands(draws) || mask.draws->command_count != draws.command_count) {
        set_error("%s: the masked draws select from other commands, or another command_count, than the opaque draws: their keys would not share one space", who);
        return UR_EINVAL;
    }
    if (!mask.keys64 || !aligned(mask.keys64, 8) || !aligned(mask.won, 4)) { set_error("%s: a null or misaligned keys64 (8 bytes) or a misaligned won (4 bytes)", who); return UR_EINVAL; }
    const size_t n = (size_t)w * rows;
    const struct { const void* at; size_t bytes; } others[] = {{targets.gbuf_a, n * 8u}, {targets.gbuf_b, n * 8u}, {targets.gbuf_c, n * 4u}, {targets.hdr, n * 8u},
                                                               {targets.keys, n * 4u}, {targets.object_id, n * 4u}, {depth, (size_t)w * h * 4u}};
    for (const auto& o : others) {
        if (o.at && overlaps(mask.keys64, n * 8u, o.at, o.bytes)) { set_error("%s: keys64 overlaps a target or depth", who); return UR_EINVAL; }
    }
    if (targets.object_id) {
        set_error("%s: object_id beside a mask: the ObjectId pass ignores the alpha test and tests against the depth this pass writes; it needs a raster of its own", who);
        return UR_EUNSUPPORTED;
    }
    return UR_OK;
}

extern "C" {

int ur_forward_pass_parts(ur_ctx* ctx, const float* view, const float* projection, const ur_raster_draws* draws, float* depth, const ur_forward_targets* targets,
                          uint32_t w, uint32_t h, uint32_t row0, uint32_t rows, uint32_t flags, uint32_t key_triangle_bits, uint32_t* stats6, uint32_t parts,
                          const ur_material* materials, uint32_t material_count, const ur_gbuffer_mask* mask, const ur_scene_constants* frame_constants,
                          const ur_lighting_tables* tables)
{
    ur_gbuffer_targets t{};
    if (targets) { t.hdr = targets->hdr; t.keys = targets->keys; }
    const ForwardCall forward{frame_constants, tables};
    return gbuffer_entry("ur_forward_pass", "ur_forward_pass_parts", ctx, view, projection, draws, depth, targets ? &t : nullptr, w, h, row0, rows, flags,
                         key_triangle_bits, stats6, parts, materials, material_count, mask, depth, &forward);
}

int ur_forward_pass(ur_ctx* ctx, const float* view, const float* projection, const ur_raster_draws* draws, float* depth, const ur_forward_targets* targets, uint32_t w,
                    uint32_t h, uint32_t row0, uint32_t rows, uint32_t flags, uint32_t key_triangle_bits, uint32_t* stats6, const ur_material* materials,
                    uint32_t material_count, const ur_gbuffer_mask* mask, const ur_scene_constants* frame_constants, const ur_lighting_tables* tables)
{
    return ur_forward_pass_parts(ctx, view, projection, draws, depth, targets, w, h, row0, rows, flags, key_triangle_bits, stats6,
                                 UR_GBUFFER_PART_RASTER | UR_GBUFFER_PART_RESOLVE, materials, material_count, mask, frame_constants, tables);
}

int ur_gbuffer_pass_masked_parts(ur_ctx* ctx, const float* view, const float* projection, const ur_raster_draws* draws, float* depth, const ur_gbuffer_targets* targets,
                                 uint32_t w, uint32_t h, uint32_t row0, uint32_t rows, uint32_t flags, uint32_t key_triangle_bits, uint32_t* stats6, uint32_t parts,
                                 const ur_material* materials, uint32_t material_count, const ur_gbuffer_mask* mask)
{
    return gbuffer_entry("ur_gbuffer_pass_masked", "ur_gbuffer_pass_masked_parts", ctx, view, projection, draws, depth, targets, w, h, row0, rows, flags, key_triangle_bits,
                         stats6, parts, materials, material_count, mask, depth);
}

int ur_gbuffer_pass_masked(ur_ctx* ctx, const float* view, const float* projection, const ur_raster_draws* draws, float* depth, const ur_gbuffer_targets* targets,
                           uint32_t w, uint32_t h, uint32_t row0, uint32_t rows, uint32_t flags, uint32_t key_triangle_bits, uint32_t* stats6,
                           const ur_material* materials, uint32_t material_count, const ur_gbuffer_mask* mask)
{
    return gbuffer_entry("ur_gbuffer_pass_masked", "ur_gbuffer_pass_masked_parts", ctx, view, projection, draws, depth, targets, w, h, row0, rows, flags, key_triangle_bits,
                         stats6, UR_GBUFFER_PART_RASTER | UR_GBUFFER_PART_RESOLVE, materials, material_count, mask, depth);
}

int ur_gbuffer_pass_materials_parts(ur_ctx* ctx, const float* view, const float* projection, const ur_raster_draws* draws, const float* depth,
                                    const ur_gbuffer_targets* targets, uint32_t w, uint32_t h, uint32_t row0, uint32_t rows, uint32_t flags, uint32_t key_triangle_bits,
                                    uint32_t* stats6, uint32_t parts, const ur_material* materials, uint32_t material_count)
{
    return gbuffer_entry("ur_gbuffer_pass_materials", "ur_gbuffer_pass_materials_parts", ctx, view, projection, draws, depth, targets, w, h, row0, rows, flags,
                         key_triangle_bits, stats6, parts, materials, material_count);
}

int ur_gbuffer_pass_materials(ur_ctx* ctx, const float* view, const float* projection, const ur_raster_draws* draws, const float* depth, const ur_gbuffer_targets* targets,
                              uint32_t w, uint32_t h, uint32_t row0, uint32_t rows, uint32_t flags, uint32_t key_triangle_bits, uint32_t* stats6,
                              const ur_material* materials, uint32_t material_count)
{
    return gbuffer_entry("ur_gbuffer_pass_materials", "ur_gbuffer_pass_materials_parts", ctx, view, projection, draws, depth, targets, w, h, row0, rows, flags,
                         key_triangle_bits, stats6, UR_GBUFFER_PART_RASTER | UR_GBUFFER_PART_RESOLVE, materials, material_count);
}

int ur_gbuffer_pass_parts(ur_ctx* ctx, const float* view, const float* projection, const ur_raster_draws* draws, const float* depth, const ur_gbuffer_targets* targets,
                          uint32_t w, uint32_t h, uint32_t row0, uint32_t rows, uint32_t flags, uint32_t key_triangle_bits, uint32_t* stats6, uint32_t parts)
{
    return gbuffer_entry("ur_gbuffer_pass", "ur_gbuffer_pass_parts", ctx, view, projection, draws, depth, targets, w, h, row0, rows, flags, key_triangle_bits, stats6, parts,
                         nullptr, 0u);
}

int ur_gbuffer_pass(ur_ctx* ctx, const float* view, const float* projection, const ur_raster_draws* draws, const float* depth, const ur_gbuffer_targets* targets,
                    uint32_t w, uint32_t h, uint32_t row0, uint32_t rows, uint32_t flags, uint32_t key_triangle_bits, uint32_t* stats6)
{
    return gbuffer_entry("ur_gbuffer_pass", "ur_gbuffer_pass_parts", ctx, view, projection, draws, depth, targets, w, h, row0, rows, flags, key_triangle_bits, stats6,
                         UR_GBUFFER_PART_RASTER | UR_GBUFFER_PART_RESOLVE, nullptr, 0u);
}

} // extern "C"

