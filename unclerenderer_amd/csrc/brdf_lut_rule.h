// The BRDF LUT (include/ur_brdf_lut.h): the split-sum table of the specular image-based lighting - the rule of the
// shipped PreintegratedGF.dds: the approximated joint Smith visibility, alpha = roughness^2, texel centres, x = NoV, y = roughness - as
// W x H texels of 2 x UNORM16 (scale | bias << 16), row-major: what ur_lighting_tables.brdf_lut_rg16 takes. This file is the rule as plain
// inline functions with no HIP intrinsic: the kernel of csrc/brdf_lut.hip calls them per lane, the serial host build
// (csrc/brdf_lut_host.cpp) and tests/cpp/env_sky_main.cpp call the same functions. fp32, uncontracted, IEEE divide and square root
// (build.py's EXACT flags); no transcendental function - those run once, on the host, in float64, for the table.
//   table    for row y and sample i (of S, section 3.20's Hammersley set) 16 bytes {hx, hy, hz, 0} in fp32: the GGX importance half vector
//            in tangent space for alpha = ((y + 0.5) / H)^2. 16 H S bytes, rows outer.
//   texel    NoV = (x + 0.5) / W, r = (y + 0.5) / H, alpha = r r, V = (sqrt(1 - NoV NoV), 0, NoV). Sample: VoH = V.x hx + V.z hz,
//            NoL = (2 VoH) hz - NoV; where NoL > 0: Vis = 0.5 / (NoL (NoV (1 - alpha) + alpha) + NoV (NoL (1 - alpha) + alpha)),
//            w = (NoL Vis) ((4 VoH) / hz), m = 1 - VoH, Fc = ((m m) (m m)) m; scale takes (1 - Fc) w, bias Fc w.
//   sum      section 3.20's order: lane j of 64 starts at +0 and adds samples j, j + 64, ... ascending, a tree over the lanes by strides
//            32 .. 1 follows; each sum times 1 / S, clamped to [0, 1], times 65535, rounded to nearest even.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "cube_sample.h" // UR_CUBE_FN
#include "ur_checks.h"   // ur::overlaps (host only, inline)

#define UR_LUT_FN UR_CUBE_FN

namespace ur_lut {

constexpr uint32_t kMaxWidth = 1024u, kMaxHeight = 256u, kMinSamples = 16u, kMaxSamples = 4096u;
constexpr uint32_t kLanes = 64u; // the lanes a texel's samples are dealt to, whatever runs them

UR_LUT_FN bool power_of_two(uint32_t v) { return v != 0u && (v & (v - 1u)) == 0u; }

inline bool valid_samples(uint32_t samples) { return power_of_two(samples) && samples >= kMinSamples && samples <= kMaxSamples; }
inline size_t table_bytes(uint32_t height, uint32_t samples)
{
    return height >= 1u && height <= kMaxHeight && valid_samples(samples) ? 16u * (size_t)height * samples : 0u;
}

// The refusals of ur_brdf_lut and ur_host_brdf_lut, from the arguments alone. Returns true (and the text) on a refusal.
inline bool refuse(const char* who, uint32_t width, uint32_t height, uint32_t samples, const void* table, size_t table_size, const void* dst, size_t dst_bytes, char* text,
                   size_t text_size)
{
    if (!table || !dst) { snprintf(text, text_size, "%s: null table or destination", who); return true; }
    if (width < 1u || width > kMaxWidth || height < 1u || height > kMaxHeight) {
        snprintf(text, text_size, "%s: a table of %u x %u (1..%u x 1..%u)", who, width, height, kMaxWidth, kMaxHeight);
        return true;
    }
    if (!valid_samples(samples)) { snprintf(text, text_size, "%s: sample count %u (a power of two, %u..%u)", who, samples, kMinSamples, kMaxSamples); return true; }
    const size_t table_need = table_bytes(height, samples), dst_need = 4u * (size_t)width * height;
    if (table_size < table_need) { snprintf(text, text_size, "%s: %zu table bytes, %zu needed (ur_brdf_lut_table_bytes)", who, table_size, table_need); return true; }
    if (dst_bytes != dst_need) { snprintf(text, text_size, "%s: %zu destination bytes, %zu expected (%u x %u texels of 2 x UNORM16)", who, dst_bytes, dst_need, width, height); return true; }
    if (reinterpret_cast<uintptr_t>(table) % 16u != 0u) { snprintf(text, text_size, "%s: table not 16-byte aligned", who); return true; }
    if (reinterpret_cast<uintptr_t>(dst) % 16u != 0u) { snprintf(text, text_size, "%s: destination not 16-byte aligned", who); return true; }
    if (ur::overlaps(table, table_size, dst, dst_bytes)) { snprintf(text, text_size, "%s: table and destination overlap", who); return true; }
    return false;
}

struct Plan {
    uint32_t width, height, samples;
    uint32_t texels;   // width * height
    float inv_samples; // 1 / samples, a power of two
};

inline Plan make_plan(uint32_t width, uint32_t height, uint32_t samples)
{
    Plan p{};
    p.width = width; p.height = height; p.samples = samples;
    p.texels = width * height;
    p.inv_samples = 1.0f / (float)samples;
    return p;
}

struct Sample { float hx, hy, hz, pad; };

// What a texel's samples share
struct Texel { float nov, vx, alpha, one_minus_alpha; uint32_t row; };

UR_LUT_FN Texel texel_of(const Plan& p, uint32_t texel)
{
    Texel t;
    t.row = texel / p.width;
    const uint32_t x = texel - t.row * p.width;
    t.nov = ((float)x + 0.5f) / (float)p.width;
    const float r = ((float)t.row + 0.5f) / (float)p.height;
    t.alpha = r * r;
    t.one_minus_alpha = 1.0f - t.alpha;
    t.vx = sqrtf(1.0f - t.nov * t.nov);
    return t;
}

// One sample added to acc = {scale, bias}
UR_LUT_FN void add_sample(const Texel& t, const Sample& s, float (&acc)[2])
{
    const float voh = t.vx * s.hx + t.nov * s.hz;
    const float nol = (2.0f * voh) * s.hz - t.nov;
    if (!(nol > 0.0f)) return; // (then voh > 0 and hz > 0 too)
    const float vis = 0.5f / (nol * (t.nov * t.one_minus_alpha + t.alpha) + t.nov * (nol * t.one_minus_alpha + t.alpha));
    const float w = (nol * vis) * ((4.0f * voh) / s.hz);
    const float m = 1.0f - voh, m2 = m * m;
    const float fc = (m2 * m2) * m;
    acc[0] = acc[0] + (1.0f - fc) * w;
    acc[1] = acc[1] + fc * w;
}

// A sum to its UNORM16 code: times 1 / S, clamped to [0, 1] (a NaN gives 0), times 65535, to nearest even
UR_LUT_FN uint32_t unorm16(float sum, float inv_samples)
{
    const float mean = sum * inv_samples;
    const float v = (mean > 0.0f ? (mean < 1.0f ? mean : 1.0f) : 0.0f) * 65535.0f;
    uint32_t q = (uint32_t)v;
    const float f = v - (float)q; // exact: v < 2^16
    if (f > 0.5f || (f == 0.5f && (q & 1u) != 0u)) ++q;
    return q;
}

UR_LUT_FN uint32_t finish(const float (&sum)[2], float inv_samples) { return unorm16(sum[0], inv_samples) | (unorm16(sum[1], inv_samples) << 16); }

// The rule, serial: texel `texel` (row-major), the 64 lanes one after the other - the kernel's wave, lane by lane
inline void texel_item(const Plan& p, const void* table, uint32_t* dst, uint32_t texel)
{
    const Texel t = texel_of(p, texel);
    const Sample* samples = static_cast<const Sample*>(table) + (size_t)t.row * p.samples;
    float lane[kLanes][2];
    for (uint32_t j = 0u; j < kLanes; ++j) {
        lane[j][0] = lane[j][1] = 0.0f;
        for (uint32_t i = j; i < p.samples; i += kLanes) add_sample(t, samples[i], lane[j]);
    }
    for (uint32_t stride = kLanes / 2u; stride != 0u; stride >>= 1)
        for (uint32_t j = 0u; j < stride; ++j)
            for (int c = 0; c < 2; ++c) lane[j][c] = lane[j][c] + lane[j + stride][c];
    dst[texel] = finish(lane[0], p.inv_samples);
}

} // namespace ur_lut
