// The environment prefilter (include/ur_env_prefilter.h): the top level of an HDR cube - six square RGBA16F faces
// of a power-of-two edge E, face-major - becomes the full prefiltered chain, L = log2(E) + 1 levels down to 1 x 1, level k filtered for
// roughness k / (L - 1): the RGBA16F payload in DDS order (face-major, mips inner) that ur_env_cube_build stages. This file is the rule as
// work items, plain inline functions with no HIP intrinsic: the kernels of csrc/env_prefilter.hip call them per lane, the serial host
// build (csrc/env_prefilter_host.cpp) and tests/cpp/env_prefilter_main.cpp call the same functions item by item. fp32, uncontracted,
// IEEE divide and square root (build.py's EXACT flags); no transcendental function - those run once, on the host, in float64, for the table.
//   top     item = one texel of level 0: the source's R, G, B and alpha 1.0, into the destination and into the pyramid.
//   down    item = one texel of pyramid level m >= 1: the 2 x 2 box mean of level m - 1, ((t00 + t10) + (t01 + t11)) * 0.25 in fp32,
//           rounded once to fp16. One launch a level: a level reads the rounded level above it.
//   stage   the pyramid (a payload in DDS order, like the destination) through ur_envc::decode_item and border_item of
//           csrc/env_cube_rule.h into bordered faces, which csrc/cube_sample.h samples as the shading does.
//   filter  one output texel of level k >= 1 = one wave: lane j of 64 adds the table's samples j, j + 64, ... ascending, a fixed tree
//           over the lanes by strides 32 .. 1 follows, then one multiply by the level's reciprocal weight and one rounding to fp16.
// Scratch: the pyramid (the destination's size), then the bordered section of the staged cube.
// The table (ur_host_env_prefilter_table): L headers of 16 bytes {fp32 1 / sum of weights, u32 samples kept, 0, 0} - level 0's is {1, 0} -
// then for every level 1 .. L - 1 its S samples of 16 bytes {lx, ly, lz, lod} in fp32: the tangent-space light vector (lz is the weight)
// and the pyramid level to sample. A dropped sample (lz <= 0) is sixteen zero bytes.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "cube_sample.h"
#include "env_cube_rule.h"

#define UR_ENVP_FN UR_CUBE_FN

namespace ur_envp {

constexpr uint32_t kMaxBase = 2048u, kMinSamples = 16u, kMaxSamples = 4096u;
constexpr uint32_t kLanes = 64u;       // the lanes a texel's samples are dealt to, whatever runs them
constexpr uint32_t kGroupTexels = 16u; // consecutive texels of one level a filter workgroup takes: four waves, four texels each
constexpr uint64_t kAlphaOne = 0x3C00ull << 48;

UR_ENVP_FN bool power_of_two(uint32_t v) { return v != 0u && (v & (v - 1u)) == 0u; }
UR_ENVP_FN uint32_t levels_of(uint32_t base) { uint32_t l = 1u; while ((base >> l) != 0u) ++l; return l; } // log2(base) + 1
// payload texels of a face in front of level m <= log2(base): sum over j < m of (base >> j)^2; and of the whole face
UR_ENVP_FN uint32_t level_start(uint32_t base, uint32_t m) { const uint32_t n = base >> m; return 4u * (base * base - n * n) / 3u; }
UR_ENVP_FN uint32_t face_texels_of(uint32_t base) { return level_start(base, levels_of(base) - 1u) + 1u; }

inline bool valid_shape(uint32_t base, uint32_t samples)
{
    return power_of_two(base) && base <= kMaxBase && power_of_two(samples) && samples >= kMinSamples && samples <= kMaxSamples;
}
inline size_t payload_bytes(uint32_t base) { return 6u * (size_t)face_texels_of(base) * 8u; } // source_bytes(kRGBA16F, base, L)
inline size_t table_bytes(uint32_t base, uint32_t samples)
{
    if (!valid_shape(base, samples)) return 0u;
    const size_t L = levels_of(base);
    return 16u * L + 16u * (size_t)samples * (L - 1u);
}
inline size_t staged_bytes(uint32_t base) { return 8u * ((size_t)ur_cube::bordered_start(base, levels_of(base) - 1u) + 54u); } // (the last level: six faces of 3 x 3)
inline size_t scratch_bytes(uint32_t base) { return power_of_two(base) && base <= kMaxBase ? payload_bytes(base) + staged_bytes(base) : 0u; }

// The refusals of ur_env_prefilter and ur_host_env_prefilter (which owns its scratch: scratch == nullptr and scratch_bytes == 0 there,
// with_scratch false), from the arguments alone. Returns true (and the text) on a refusal.
inline bool refuse(const char* who, const void* src, size_t src_bytes, uint32_t base, uint32_t samples, const void* table, size_t table_size, const void* dst,
                   size_t dst_bytes, const void* scratch, size_t scratch_size, bool with_scratch, char* text, size_t text_size)
{
    if (!src || !table || !dst || (with_scratch && !scratch)) { snprintf(text, text_size, "%s: null source, table, destination or scratch", who); return true; }
    if (!power_of_two(base) || base > kMaxBase) { snprintf(text, text_size, "%s: base size %u (a power of two, 1..%u)", who, base, kMaxBase); return true; }
    if (!power_of_two(samples) || samples < kMinSamples || samples > kMaxSamples) {
        snprintf(text, text_size, "%s: sample count %u (a power of two, %u..%u)", who, samples, kMinSamples, kMaxSamples);
        return true;
    }
    const size_t src_need = 48u * (size_t)base * base, dst_need = payload_bytes(base), table_need = table_bytes(base, samples), scratch_need = scratch_bytes(base);
    if (src_bytes != src_need) { snprintf(text, text_size, "%s: %zu source bytes, %zu expected (six faces of %u x %u RGBA16F texels)", who, src_bytes, src_need, base, base); return true; }
    if (dst_bytes != dst_need) { snprintf(text, text_size, "%s: %zu destination bytes, %zu expected (ur_env_cube_source_bytes)", who, dst_bytes, dst_need); return true; }
    if (table_size < table_need) { snprintf(text, text_size, "%s: %zu table bytes, %zu needed (ur_env_prefilter_table_bytes)", who, table_size, table_need); return true; }
    if (with_scratch && scratch_size < scratch_need) { snprintf(text, text_size, "%s: %zu scratch bytes, %zu needed (ur_env_prefilter_scratch_bytes)", who, scratch_size, scratch_need); return true; }
    const struct { const char* name; const void* p; size_t bytes; } r[4] = {{"source", src, src_bytes}, {"table", table, table_size}, {"destination", dst, dst_bytes}, {"scratch", scratch, scratch_size}};
    const int count = with_scratch ? 4 : 3;
    for (int i = 0; i < count; ++i)
        if (reinterpret_cast<uintptr_t>(r[i].p) % 16u != 0u) { snprintf(text, text_size, "%s: %s not 16-byte aligned", who, r[i].name); return true; }
    for (int i = 0; i < count; ++i)
        for (int j = i + 1; j < count; ++j)
            if (ur::overlaps(r[i].p, r[i].bytes, r[j].p, r[j].bytes)) { snprintf(text, text_size, "%s: %s and %s overlap", who, r[i].name, r[j].name); return true; }
    return false;
}

// ---- the plan
struct Plan {
    uint32_t base, levels, samples;
    uint32_t face_texels;                    // payload texels a face
    uint32_t groups;                         // filter groups of the whole chain
    uint32_t group_start[ur_envc::kLevels];  // filter groups in front of level k (levels 0 and 1: none); behind the chain: groups
};

inline Plan make_plan(uint32_t base, uint32_t samples)
{
    Plan p{};
    p.base = base; p.levels = levels_of(base); p.samples = samples;
    p.face_texels = face_texels_of(base);
    uint32_t groups = 0u;
    for (uint32_t k = 0u; k < ur_envc::kLevels; ++k) {
        p.group_start[k] = groups;
        if (k == 0u || k >= p.levels) continue;
        const uint32_t n = base >> k;
        groups += (6u * n * n + kGroupTexels - 1u) / kGroupTexels;
    }
    p.groups = groups;
    return p;
}

// ---- the items. Payloads and the staged cube are 64-bit texels (R | G << 16 | B << 32 | A << 48).
// top: item < 6 * base^2
UR_ENVP_FN void top_item(const Plan& p, const uint64_t* src, uint64_t* dst, uint64_t* pyramid, uint32_t item)
{
    const uint32_t area = p.base * p.base, face = item / area, t = item - face * area;
    const uint64_t v = (src[item] & 0x0000FFFFFFFFFFFFull) | kAlphaOne;
    const size_t at = (size_t)face * p.face_texels + t;
    dst[at] = v;
    pyramid[at] = v;
}

// down: level m >= 1, item < 6 * (base >> m)^2. Reads level m - 1 of the pyramid, writes level m.
UR_ENVP_FN void down_item(const Plan& p, uint64_t* pyramid, uint32_t m, uint32_t item)
{
    const uint32_t n = p.base >> m, area = n * n, face = item / area, t = item - face * area, y = t / n, x = t - y * n;
    const uint64_t* above = pyramid + ((size_t)face * p.face_texels + level_start(p.base, m - 1u)) + ((size_t)(2u * y) * (2u * n) + 2u * x);
    const uint64_t t00 = above[0], t10 = above[1], t01 = above[2u * n], t11 = above[2u * n + 1u];
    uint64_t v = kAlphaOne;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t c = 0u; c < 3u; ++c) {
        const uint32_t sh = 16u * c;
        const float a = ur_cube::half_value((uint32_t)(t00 >> sh) & 0xFFFFu), b = ur_cube::half_value((uint32_t)(t10 >> sh) & 0xFFFFu);
        const float d = ur_cube::half_value((uint32_t)(t01 >> sh) & 0xFFFFu), e = ur_cube::half_value((uint32_t)(t11 >> sh) & 0xFFFFu);
        v |= (uint64_t)ur_cube::half_bits(((a + b) + (d + e)) * 0.25f) << sh;
    }
    pyramid[(size_t)face * p.face_texels + level_start(p.base, m) + t] = v;
}

// ---- the filter
struct Sample { float lx, ly, lz, lod; };
struct Frame { float n[3], t[3], b[3]; };

// The direction of texel (x, y)'s centre on a face of edge n, by the inverse of ur_cube::cube_face's mapping, normalised:
//   +X (1, -t, -s)  -X (-1, -t, s)  +Y (s, 1, t)  -Y (s, -1, -t)  +Z (s, -t, 1)  -Z (-s, -t, -1),  s = (2 x + 1) / n - 1, t = (2 y + 1) / n - 1
// and the frame around it (Duff et al., "Building an Orthonormal Basis, Revisited"): +, -, *, / and copysign alone.
UR_ENVP_FN Frame texel_frame(uint32_t face, uint32_t x, uint32_t y, uint32_t n)
{
    const float s = (float)(2u * x + 1u) / (float)n - 1.0f, t = (float)(2u * y + 1u) / (float)n - 1.0f;
    const float dx = face == 0u ? 1.0f : (face == 1u ? -1.0f : (face == 5u ? -s : s));
    const float dy = face == 2u ? 1.0f : (face == 3u ? -1.0f : -t);
    const float dz = face == 0u ? -s : (face == 1u ? s : (face == 2u ? t : (face == 3u ? -t : (face == 4u ? 1.0f : -1.0f))));
    const float len = sqrtf((dx * dx + dy * dy) + dz * dz);
    Frame f;
    f.n[0] = dx / len; f.n[1] = dy / len; f.n[2] = dz / len;
    const float sign = copysignf(1.0f, f.n[2]);
    const float a = -1.0f / (sign + f.n[2]);
    const float b = (f.n[0] * f.n[1]) * a;
    f.t[0] = 1.0f + sign * ((f.n[0] * f.n[0]) * a); f.t[1] = sign * b; f.t[2] = -(sign * f.n[0]);
    f.b[0] = b; f.b[1] = sign + (f.n[1] * f.n[1]) * a; f.b[2] = -f.n[1];
    return f;
}

// One kept sample (lz > 0): the light vector in the frame, one sample of the staged pyramid at its level, lz * rgb added to acc.
UR_ENVP_FN void add_sample(const Plan& p, const uint64_t* staged, const Frame& f, const Sample& s, float (&acc)[3])
{
    float d[3], rgb[3];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int c = 0; c < 3; ++c) d[c] = (f.t[c] * s.lx + f.b[c] * s.ly) + f.n[c] * s.lz;
    ur_cube::cube_sample_level(staged, p.base, p.levels, d, s.lod, rgb);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int c = 0; c < 3; ++c) acc[c] = acc[c] + s.lz * rgb[c];
}

// Where level k's texel `t` (of 6 * (base >> k)^2, face-major) lies: its face and coordinates, and its place in the payload
struct Place { uint32_t face, x, y, n; size_t at; };
UR_ENVP_FN Place place_of(const Plan& p, uint32_t k, uint32_t t)
{
    Place o;
    o.n = p.base >> k;
    const uint32_t area = o.n * o.n, rest = t - (t / area) * area;
    o.face = t / area; o.y = rest / o.n; o.x = rest - o.y * o.n;
    o.at = (size_t)o.face * p.face_texels + level_start(p.base, k) + rest;
    return o;
}

// The texel a sum becomes: one multiply by the level's reciprocal weight, one rounding
UR_ENVP_FN uint64_t finish(const float (&sum)[3], float inv_weight)
{
    return kAlphaOne | (uint64_t)ur_cube::half_bits(sum[0] * inv_weight) | ((uint64_t)ur_cube::half_bits(sum[1] * inv_weight) << 16) |
           ((uint64_t)ur_cube::half_bits(sum[2] * inv_weight) << 32);
}

// filter, serial: texel t of level k >= 1, the lanes one after the other. `table` is the whole table.
inline void filter_item(const Plan& p, const uint64_t* staged, const void* table, uint64_t* dst, uint32_t k, uint32_t t)
{
    const float* header = static_cast<const float*>(table) + 4u * (size_t)k;
    const Sample* samples = reinterpret_cast<const Sample*>(static_cast<const char*>(table) + 16u * (size_t)p.levels) + (size_t)(k - 1u) * p.samples;
    const Place o = place_of(p, k, t);
    const Frame f = texel_frame(o.face, o.x, o.y, o.n);
    float lane[kLanes][3];
    for (uint32_t j = 0u; j < kLanes; ++j) {
        lane[j][0] = lane[j][1] = lane[j][2] = 0.0f;
        for (uint32_t i = j; i < p.samples; i += kLanes)
            if (samples[i].lz > 0.0f) add_sample(p, staged, f, samples[i], lane[j]);
    }
    for (uint32_t stride = kLanes / 2u; stride != 0u; stride >>= 1)
        for (uint32_t j = 0u; j < stride; ++j)
            for (int c = 0; c < 3; ++c) lane[j][c] = lane[j][c] + lane[j + stride][c];
    dst[o.at] = finish(lane[0], header[0]);
}

} // namespace ur_envp
