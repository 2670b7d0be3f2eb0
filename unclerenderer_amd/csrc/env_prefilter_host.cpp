// ur_host_env_prefilter_table, ur_host_env_prefilter and the two size functions (include/ur_host.h, include/ur_env_prefilter.h): the
// environment prefilter of DESIGN.md section 3.20 in plain serial C++ over csrc/env_prefilter_rule.h - the items the kernels of
// csrc/env_prefilter.hip run, launch by launch - and the one place its transcendental functions run: the table, in double. Any compiler
// builds it; it is the CPU fallback and the byte reference of the device build.

#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/ur_host.h"
#include "env_prefilter_rule.h"

extern "C" size_t ur_env_prefilter_table_bytes(uint32_t base_size, uint32_t sample_count) { return ur_envp::table_bytes(base_size, sample_count); }
extern "C" size_t ur_env_prefilter_scratch_bytes(uint32_t base_size) { return ur_envp::scratch_bytes(base_size); }

extern "C" int ur_host_env_prefilter_table(uint32_t base_size, uint32_t sample_count, void* out, size_t out_bytes)
{
    using namespace ur_envp;
    const size_t need = table_bytes(base_size, sample_count);
    if (!out || need == 0u || out_bytes < need) return UR_EINVAL;
    const uint32_t L = levels_of(base_size), S = sample_count;
    const double pi = 3.14159265358979323846;
    const double omega_p = 4.0 * pi / (6.0 * (double)base_size * (double)base_size);
    char* bytes = static_cast<char*>(out);
    std::memset(bytes, 0, need);
    const float one = 1.0f;
    std::memcpy(bytes, &one, 4);
    for (uint32_t k = 1u; k < L; ++k) {
        const double r = (double)k / (double)(L - 1u), alpha = r * r, a2 = alpha * alpha;
        double weight = 0.0;
        uint32_t kept = 0u;
        char* level = bytes + 16u * (size_t)L + 16u * (size_t)S * (k - 1u);
        for (uint32_t i = 0u; i < S; ++i) {
            uint32_t b = i; // the radical inverse of i in base 2
            b = (b << 16) | (b >> 16);
            b = ((b & 0x00FF00FFu) << 8) | ((b & 0xFF00FF00u) >> 8);
            b = ((b & 0x0F0F0F0Fu) << 4) | ((b & 0xF0F0F0F0u) >> 4);
            b = ((b & 0x33333333u) << 2) | ((b & 0xCCCCCCCCu) >> 2);
            b = ((b & 0x55555555u) << 1) | ((b & 0xAAAAAAAAu) >> 1);
            const double xi1 = (double)i / (double)S, xi2 = (double)b * (1.0 / 4294967296.0);
            const double cos2 = (1.0 - xi2) / (1.0 + (a2 - 1.0) * xi2), hz = std::sqrt(cos2), sine = std::sqrt(1.0 - cos2);
            const double phi = 2.0 * pi * xi1, hx = sine * std::cos(phi), hy = sine * std::sin(phi);
            const double t = cos2 * (a2 - 1.0) + 1.0, D = a2 / (pi * t * t);
            const double omega_s = 4.0 / ((double)S * D);
            double lod = 0.5 * std::log2(omega_s / omega_p); // (no constant on top: DESIGN.md 3.20 has the measurement)
            lod = lod < 0.0 ? 0.0 : (lod > (double)(L - 1u) ? (double)(L - 1u) : lod);
            const Sample s = {(float)(2.0 * hz * hx), (float)(2.0 * hz * hy), (float)(2.0 * cos2 - 1.0), (float)lod};
            if (!(s.lz > 0.0f)) continue; // dropped: sixteen zero bytes
            std::memcpy(level + 16u * (size_t)i, &s, 16);
            weight += (double)s.lz;
            ++kept;
        }
        const float inv = (float)(1.0 / weight);
        std::memcpy(bytes + 16u * (size_t)k, &inv, 4);
        std::memcpy(bytes + 16u * (size_t)k + 4u, &kept, 4);
    }
    return UR_OK;
}

extern "C" int ur_host_env_prefilter(const void* src_host, size_t src_bytes, uint32_t base_size, uint32_t sample_count, const void* table_host, size_t table_size,
                                     void* dst_host, size_t dst_bytes)
{
    using namespace ur_envp;
    char text[256];
    if (refuse("ur_host_env_prefilter", src_host, src_bytes, base_size, sample_count, table_host, table_size, dst_host, dst_bytes, nullptr, 0u, false, text, sizeof text))
        return UR_EINVAL;
    const Plan p = make_plan(base_size, sample_count);
    std::vector<uint64_t> pyramid(payload_bytes(base_size) / 8u), staged(staged_bytes(base_size) / 8u);
    const uint64_t* src = static_cast<const uint64_t*>(src_host);
    uint64_t* dst = static_cast<uint64_t*>(dst_host);
    for (uint32_t item = 0u; item < 6u * base_size * base_size; ++item) top_item(p, src, dst, pyramid.data(), item);
    for (uint32_t m = 1u; m < p.levels; ++m)
        for (uint32_t item = 0u; item < 6u * (base_size >> m) * (base_size >> m); ++item) down_item(p, pyramid.data(), m, item);
    const ur_envc::Plan stage = ur_envc::make_plan(ur_envc::kRGBA16F, base_size, p.levels);
    for (uint32_t item = 0u; item < 6u * stage.decode_face; ++item) ur_envc::decode_item(stage, pyramid.data(), staged.data(), item, false, false, nullptr);
    for (uint32_t item = 0u; item < 6u * stage.border_face; ++item) ur_envc::border_item(stage, staged.data(), item);
    for (uint32_t k = 1u; k < p.levels; ++k)
        for (uint32_t t = 0u; t < 6u * (base_size >> k) * (base_size >> k); ++t) filter_item(p, staged.data(), table_host, dst, k, t);
    return UR_OK;
}
