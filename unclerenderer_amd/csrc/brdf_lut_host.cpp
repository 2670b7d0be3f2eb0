// ur_brdf_lut_table_bytes, ur_host_brdf_lut_table and ur_host_brdf_lut (include/ur_brdf_lut.h, include/ur_host.h): the BRDF LUT of
// DESIGN.md section 3.22 in plain serial C++ over csrc/brdf_lut_rule.h - the functions the kernel of csrc/brdf_lut.hip runs, texel by
// texel in the rule's own 64-lane order - and the one place its transcendental functions run: the table, in double. Any compiler builds
// it; it is the CPU fallback and the byte reference of the device build.

#include <cmath>
#include <cstring>

#include "../../include/ur_host.h"
#include "brdf_lut_rule.h"

extern "C" size_t ur_brdf_lut_table_bytes(uint32_t height, uint32_t sample_count) { return ur_lut::table_bytes(height, sample_count); }

extern "C" int ur_host_brdf_lut_table(uint32_t height, uint32_t sample_count, void* out, size_t out_bytes)
{
    using namespace ur_lut;
    const size_t need = table_bytes(height, sample_count);
    if (!out || need == 0u || out_bytes < need) return UR_EINVAL;
    const uint32_t S = sample_count;
    const double pi = 3.14159265358979323846;
    char* bytes = static_cast<char*>(out);
    for (uint32_t y = 0u; y < height; ++y) {
        const double r = ((double)y + 0.5) / (double)height, alpha = r * r, a2 = alpha * alpha;
        for (uint32_t i = 0u; i < S; ++i) {
            uint32_t b = i; // the radical inverse of i in base 2
            b = (b << 16) | (b >> 16);
            b = ((b & 0x00FF00FFu) << 8) | ((b & 0xFF00FF00u) >> 8);
            b = ((b & 0x0F0F0F0Fu) << 4) | ((b & 0xF0F0F0F0u) >> 4);
            b = ((b & 0x33333333u) << 2) | ((b & 0xCCCCCCCCu) >> 2);
            b = ((b & 0x55555555u) << 1) | ((b & 0xAAAAAAAAu) >> 1);
            const double xi1 = (double)i / (double)S, xi2 = (double)b * (1.0 / 4294967296.0);
            const double cos2 = (1.0 - xi2) / (1.0 + (a2 - 1.0) * xi2), hz = std::sqrt(cos2), sine = std::sqrt(1.0 - cos2);
            const double phi = 2.0 * pi * xi1;
            const Sample s = {(float)(sine * std::cos(phi)), (float)(sine * std::sin(phi)), (float)hz, 0.0f};
            std::memcpy(bytes + 16u * ((size_t)y * S + i), &s, 16);
        }
    }
    return UR_OK;
}

extern "C" int ur_host_brdf_lut(uint32_t width, uint32_t height, uint32_t sample_count, const void* table_host, size_t table_size, void* dst_host, size_t dst_bytes)
{
    using namespace ur_lut;
    char text[256];
    if (refuse("ur_host_brdf_lut", width, height, sample_count, table_host, table_size, dst_host, dst_bytes, text, sizeof text)) return UR_EINVAL;
    const Plan p = make_plan(width, height, sample_count);
    uint32_t* dst = static_cast<uint32_t*>(dst_host);
    for (uint32_t texel = 0u; texel < p.texels; ++texel) texel_item(p, table_host, dst, texel);
    return UR_OK;
}
