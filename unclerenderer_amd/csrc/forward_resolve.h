// The Forward pass' resolve (csrc/forward_resolve.hip): its launch arguments, filled in by the entry points beside GBuffer's launch code
// (csrc/gbuffer_resolve.hip). Not installed.
#pragma once

#include "ur_internal.h"

namespace ur {

struct ForwardParams {
    // ---- the keys and the draws behind them: csrc/gbuffer_resolve.hip's ResolveParams
    const uint8_t* commands;
    uint32_t mode; // 0 every slot / ranges (the ordinal is the slot), 1 list (the ordinal is the position in the list)
    const uint32_t* visible_idx;
    uint32_t index_base;
    float V[16], Pr[16];
    const uint32_t* keys;
    uint2* hdr;
    uint32_t w, row0, n; // n = rows * w
    float half_w, half_h;
    uint32_t key_bits;
    const ur_material* materials;
    uint32_t material_count;
    const float* decode; // 256 entries of the sRGB decode
    const float* lod;    // 127 thresholds of the level of detail
    const unsigned long long* keys64;
    const uint32_t* mask_visible_idx;
    uint32_t mask_mode, mask_index_base;
    // ---- the per-frame constants, as frame_constants holds them
    float camera[3], light_direction[3], light_color[3], light_intensity;
    float lvp[16];
    float shadow_strength, shadow_bias, shadow_size[2];
    float max_mip; // max(0, EnvMapMipCount - 1)
    // ---- the lighting tables
    const float* shadow;
    int shadow_w, shadow_h;
    const uint2* env; // the bordered faces of the staged cube
    uint32_t env_base, env_mips;
    uint32_t env_offset[16]; // where mip m's bordered faces start, in texels
    const uint32_t* lut;
    uint32_t lut_w, lut_h;
};

// maps: the textured kernel (materials is not null); masked: the one that finds a masked key's slot through keys64
int launch_forward_resolve(ur_ctx* ctx, const ForwardParams& p, bool maps, bool masked);

} // namespace ur
