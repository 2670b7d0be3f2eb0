// ur_host_env_cube_build and ur_env_cube_source_bytes (include/ur_host.h, include/ur_env_cube.h): the environment cube build of DESIGN.md
// section 3.19 in plain serial C++ - the payload walked face by face, mips inner, block by block with csrc/bc6h_decode.h, the decoder the
// kernels of csrc/env_cube_build.hip run, then ur::stage_env_cube_host (csrc/env_cube_stage.cpp), the function ur_stage_env_cube runs.
// Any compiler builds it (with env_cube_stage.cpp and lighting_plan.cpp); it is the CPU fallback and the byte reference of the device build.

#include <cstring>
#include <vector>

#include "../../include/ur_host.h"
#include "env_cube_rule.h"

extern "C" size_t ur_env_cube_source_bytes(uint32_t format, uint32_t base_size, uint32_t mip_count) { return ur_envc::source_bytes(format, base_size, mip_count); }

extern "C" int ur_host_env_cube_build(const void* src_host, size_t src_bytes, uint32_t format, uint32_t base_size, uint32_t mip_count, ur_half4* dst_host,
                                      size_t dst_texels, uint32_t* reserved_blocks)
{
    using namespace ur_envc;
    char text[256];
    if (refuse("ur_host_env_cube_build", src_host, src_bytes, format, base_size, mip_count, dst_host, dst_texels, reserved_blocks, text, sizeof text)) return UR_EINVAL;
    const ur::CubeLayout L = ur::cube_layout(base_size, mip_count);
    size_t face_texels = 0u;
    for (uint32_t m = 0u; m < mip_count; ++m) face_texels += (size_t)level_size(base_size, m) * level_size(base_size, m);
    std::vector<ur_half4> texels(6u * face_texels);
    const uint8_t* src = static_cast<const uint8_t*>(src_host);
    ur_half4* out = texels.data();
    uint32_t bad = 0u;
    for (uint32_t face = 0u; face < 6u; ++face)
        for (uint32_t m = 0u; m < mip_count; ++m) {
            const uint32_t n = level_size(base_size, m);
            if (!is_bc6h(format)) {
                std::memcpy(out, src, (size_t)n * n * 8u);
                src += (size_t)n * n * 8u;
            } else {
                const uint32_t across = blocks_across(n);
                for (uint32_t by = 0u; by < across; ++by)
                    for (uint32_t bx = 0u; bx < across; ++bx, src += 16) {
                        uint64_t lo, hi;
                        std::memcpy(&lo, src, 8);
                        std::memcpy(&hi, src + 8, 8);
                        ur_bc6h::Header h;
                        const bool ok = ur_bc6h::decode_header(lo, hi, format == kSF16, h);
                        if (!ok) ++bad;
                        for (uint32_t t = 0u; t < 16u; ++t) {
                            const uint32_t x = bx * 4u + (t & 3u), y = by * 4u + (t >> 2);
                            if (x >= n || y >= n) continue;
                            const uint64_t v = ok ? ur_bc6h::texel(h, lo, hi, t, format == kSF16, &ur_bc6h::kTables) : ur_bc6h::kReservedTexel;
                            std::memcpy(&out[(size_t)y * n + x], &v, 8);
                        }
                    }
            }
            out += (size_t)n * n;
        }
    ur::stage_env_cube_host(texels.data(), L, dst_host);
    if (reserved_blocks) *reserved_blocks = bad;
    return UR_OK;
}
