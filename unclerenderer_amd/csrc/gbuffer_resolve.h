// The launch arguments of GBuffer's resolve (csrc/gbuffer_resolve.hip) and the part of them that the Forward pass' resolve shares
// (csrc/forward_resolve.h), filled in by the entry points (csrc/gbuffer_api.hip). Not installed.
#pragma once

#include "ur_internal.h"

namespace ur {

// What csrc/visibility_key.h reads to take a texel's key back to its draw and its material: the leading part of both resolves' arguments
struct KeyParams {
    const uint8_t* commands;
    uint32_t mode; // 0 every slot / ranges (the ordinal is the slot), 1 list (the ordinal is the position in the list)
    const uint32_t* visible_idx;
    uint32_t index_base;
    float V[16], Pr[16];
    const uint32_t* keys;
    uint32_t w, row0, n; // n = rows * w
    float half_w, half_h;
    uint32_t key_bits;
    // the textured resolves
    const ur_material* materials;
    uint32_t material_count;
    const float* decode; // 256 entries of the sRGB decode
    const float* lod;    // 127 thresholds of the level of detail
    // with masked draws under visible lists: a texel's key is a position in the masked list iff its word is not 0
    const unsigned long long* keys64;
    const uint32_t* mask_visible_idx;
    uint32_t mask_mode, mask_index_base;
};

struct ResolveParams : KeyParams {
    uint2* gbuf_a; uint2* gbuf_b; uint32_t* gbuf_c; uint2* hdr; uint32_t* object_id;
    const float* table; // 255 thresholds of the sRGB encode
};

// object_id: the kernel that writes the ObjectId target too; maps: the textured kernel (materials is not null); masked: the one that finds
// a masked key's slot through keys64 (never beside object_id: check_gbuffer_mask refuses the pair)
int launch_gbuffer_resolve(ur_ctx* ctx, const ResolveParams& p, bool object_id, bool maps, bool masked);

// The ObjectId pass' resolve: what of a KeyParams takes a key to its command, and the one target
struct ObjectIdParams {
    const uint8_t* commands;
    uint32_t mode; // as KeyParams'
    const uint32_t* visible_idx;
    uint32_t index_base;
    const uint32_t* keys;
    uint32_t n, key_bits;
    uint32_t* object_id;
};

int launch_object_id_resolve(ur_ctx* ctx, const ObjectIdParams& p);

} // namespace ur
