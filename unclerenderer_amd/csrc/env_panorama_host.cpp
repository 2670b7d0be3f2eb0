// ur_host_env_panorama and ur_host_env_panorama_taps (include/ur_host.h): the environment from a panorama of DESIGN.md section 3.21 in
// plain serial C++ over csrc/env_panorama_rule.h - the functions the kernel of csrc/env_panorama.hip runs, texel by texel in the rule's
// own 64-lane order. Any compiler builds it; it is the CPU fallback and the byte reference of the device build.

#include "../../include/ur_host.h"
#include "env_panorama_rule.h"

extern "C" uint32_t ur_host_env_panorama_taps(uint32_t width, uint32_t height, uint32_t base_size) { return ur_pano::recommended_taps(width, height, base_size); }

extern "C" int ur_host_env_panorama(const void* rgbe_host, size_t rgbe_bytes, uint32_t width, uint32_t height, uint32_t base_size, uint32_t taps, void* dst_host,
                                    size_t dst_bytes)
{
    using namespace ur_pano;
    char text[256];
    if (refuse("ur_host_env_panorama", rgbe_host, rgbe_bytes, width, height, base_size, taps, dst_host, dst_bytes, text, sizeof text)) return UR_EINVAL;
    const Plan p = make_plan(width, height, base_size, taps);
    const uint32_t* rgbe = static_cast<const uint32_t*>(rgbe_host);
    uint64_t* dst = static_cast<uint64_t*>(dst_host);
    for (uint32_t texel = 0u; texel < p.texels; ++texel) texel_item(p, rgbe, dst, texel);
    return UR_OK;
}
