// ur_host_env_sky_params and ur_host_env_sky (include/ur_host.h): the sky capture of DESIGN.md section 3.22 in plain serial C++ over
// csrc/env_sky_rule.h - the functions the kernel of csrc/env_sky.hip runs, texel by texel in the rule's own 64-lane order - and the fold
// of the constants in double, which ur_env_sky runs too. Any compiler builds it; it is the CPU fallback and the byte reference of the
// device build.

#include <cstring>

#include "../../include/ur_host.h"
#include "env_sky_rule.h"

extern "C" int ur_host_env_sky_params(const ur_sky_constants* sky, float out[10])
{
    char text[256];
    if (!sky || !out || ur_sky::refuse_constants("ur_host_env_sky_params", sky->CameraPosition, sky->LightDirection, sky->LightColor, text, sizeof text)) return UR_EINVAL;
    const ur_sky::Params p = ur_sky::fold(sky->CameraPosition, sky->LightDirection, sky->LightColor);
    static_assert(sizeof(ur_sky::Params) == 40, "ten floats");
    std::memcpy(out, &p, sizeof p);
    return UR_OK;
}

extern "C" int ur_host_env_sky(const ur_sky_constants* sky, uint32_t base_size, uint32_t taps, void* dst_host, size_t dst_bytes)
{
    using namespace ur_sky;
    char text[256];
    if (!sky || refuse("ur_host_env_sky", base_size, taps, dst_host, dst_bytes, text, sizeof text) ||
        refuse_constants("ur_host_env_sky", sky->CameraPosition, sky->LightDirection, sky->LightColor, text, sizeof text))
        return UR_EINVAL;
    const Plan p = make_plan(fold(sky->CameraPosition, sky->LightDirection, sky->LightColor), base_size, taps);
    uint64_t* dst = static_cast<uint64_t*>(dst_host);
    for (uint32_t texel = 0u; texel < p.texels; ++texel) texel_item(p, dst, texel);
    return UR_OK;
}
