// The Forward pass' resolve (csrc/forward_resolve.hip): its launch arguments, filled in by the entry points it shares with the GBuffer pass
// (csrc/gbuffer_api.hip). Not installed.
#pragma once

#include "gbuffer_resolve.h"

namespace ur {

struct ForwardParams : KeyParams {
    uint2* hdr;
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
