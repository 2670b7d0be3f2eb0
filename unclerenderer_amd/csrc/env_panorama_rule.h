// The environment from a panorama (include/ur_env_panorama.h): W x H RGBE texels of a lat-long Radiance panorama
// - the bytes ur_hdr_unpack leaves, top row first - become the top level of an HDR cube, six square RGBA16F faces of a power-of-two edge E,
// face-major, alpha 1.0: exactly ur_env_prefilter's source. This file is the rule as plain inline functions with no HIP intrinsic: the
// kernel of csrc/env_panorama.hip calls them per lane, the serial host build (csrc/env_panorama_host.cpp) and
// tests/cpp/env_panorama_main.cpp call the same functions. fp32, uncontracted, IEEE divide and square root (build.py's EXACT flags); no
// libm function on the device: atan2 is written out below.
//   texel    m * 2^(e - 136) per channel, 0 when e == 0 (stb_image's convention), built in integers: every such value is exact in fp32, some
//            as subnormals.
//   tap      sub-sample (sx, sy) of K x K of output texel (x, y): s = (2 (x K + sx) + 1) / (K E) - 1, t likewise, the direction by section
//            3.20's face table, u = 0.5 + atan2(dx, dz) / 2 pi, v = 0.5 - atan2(dy, sqrt(dx^2 + dz^2)) / pi, one bilinear sample of the
//            panorama at (u W - 0.5, v H - 0.5): columns wrap, rows clamp.
//   sum      section 3.20's order: tap i = sy K + sx; lane j of 64 starts at +0 and adds taps j, j + 64, ... ascending, a tree over the
//            lanes by strides 32 .. 1 follows, lane 0 times 1 / K^2, min(., 65504), one rounding to fp16.
// Every tap is >= +0, so adding an idle lane's +0 changes nothing: a wave may hold 64 / K^2 texels when K^2 < 64 and run only the strides
// below K^2 (wave_item below, the kernel's shape). The bytes are texel_item's.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "cube_sample.h" // ur_cube::half_bits
#include "ur_checks.h"   // ur::overlaps (host only, inline)

#define UR_PANO_FN UR_CUBE_FN

namespace ur_pano {

constexpr uint32_t kMaxWidth = 16384u, kMaxHeight = 8192u, kMaxBase = 2048u, kMaxTaps = 16u;
constexpr uint32_t kLanes = 64u; // the lanes a texel's taps are dealt to, whatever runs them
constexpr uint64_t kAlphaOne = 0x3C00ull << 48;
constexpr float kHalfMax = 65504.0f;

UR_PANO_FN bool power_of_two(uint32_t v) { return v != 0u && (v & (v - 1u)) == 0u; }

// The smallest power of two K with 3 K E >= 2 W and 3 K E >= 4 H, at most 16: sub-samples at most about half a panorama texel apart at
// a face's centre (there ds = 2 / (K E) is an angle of 2 / (K E) rad, a texel is 2 pi / W rad wide and pi / H rad high). 0 for sizes the
// call refuses.
inline uint32_t recommended_taps(uint32_t width, uint32_t height, uint32_t base)
{
    if (width < 1u || width > kMaxWidth || height < 1u || height > kMaxHeight || !power_of_two(base) || base > kMaxBase) return 0u;
    uint32_t k = 1u;
    while (k < kMaxTaps && (3u * k * base < 2u * width || 3u * k * base < 4u * height)) k *= 2u;
    return k;
}

// The refusals of ur_env_panorama and ur_host_env_panorama, from the arguments alone. Returns true (and the text) on a refusal.
inline bool refuse(const char* who, const void* src, size_t src_bytes, uint32_t width, uint32_t height, uint32_t base, uint32_t taps, const void* dst, size_t dst_bytes,
                   char* text, size_t text_size)
{
    if (!src || !dst) { snprintf(text, text_size, "%s: null source or destination", who); return true; }
    if (width < 1u || width > kMaxWidth || height < 1u || height > kMaxHeight) {
        snprintf(text, text_size, "%s: a panorama of %u x %u (1..%u x 1..%u)", who, width, height, kMaxWidth, kMaxHeight);
        return true;
    }
    if (!power_of_two(base) || base > kMaxBase) { snprintf(text, text_size, "%s: base size %u (a power of two, 1..%u)", who, base, kMaxBase); return true; }
    if (!power_of_two(taps) || taps > kMaxTaps) { snprintf(text, text_size, "%s: %u taps a side (a power of two, 1..%u)", who, taps, kMaxTaps); return true; }
    const size_t src_need = 4u * (size_t)width * height, dst_need = 48u * (size_t)base * base;
    if (src_bytes != src_need) { snprintf(text, text_size, "%s: %zu source bytes, %zu expected (%u x %u RGBE texels)", who, src_bytes, src_need, width, height); return true; }
    if (dst_bytes != dst_need) { snprintf(text, text_size, "%s: %zu destination bytes, %zu expected (six faces of %u x %u RGBA16F texels)", who, dst_bytes, dst_need, base, base); return true; }
    if (reinterpret_cast<uintptr_t>(src) % 4u != 0u) { snprintf(text, text_size, "%s: source not 4-byte aligned", who); return true; }
    if (reinterpret_cast<uintptr_t>(dst) % 16u != 0u) { snprintf(text, text_size, "%s: destination not 16-byte aligned", who); return true; }
    if (ur::overlaps(src, src_bytes, dst, dst_bytes)) { snprintf(text, text_size, "%s: source and destination overlap", who); return true; }
    return false;
}

// ---- the plan
struct Plan {
    uint32_t width, height, base, taps;
    uint32_t taps2_log2;  // log2(taps^2): 0, 2, 4, 6, 8
    uint32_t texels;      // 6 base^2
    uint32_t wave_texels; // the texels a wave holds: 64 / taps^2, at least 1
    uint32_t waves;
    float inv_taps2;      // 1 / taps^2, a power of two
};

inline Plan make_plan(uint32_t width, uint32_t height, uint32_t base, uint32_t taps)
{
    Plan p{};
    p.width = width; p.height = height; p.base = base; p.taps = taps;
    while ((1u << p.taps2_log2) < taps * taps) ++p.taps2_log2;
    p.texels = 6u * base * base;
    p.wave_texels = taps * taps < kLanes ? kLanes / (taps * taps) : 1u;
    p.waves = (p.texels + p.wave_texels - 1u) / p.wave_texels;
    p.inv_taps2 = 1.0f / (float)(taps * taps);
    return p;
}

// ---- the texel: m * 2^(e - 136) as an fp32, exact. With m's top bit at p the value is 1.f * 2^(p + e - 136): the biased exponent
// p + e - 9 when that is at least 1, else a subnormal of m << (e + 13) units of 2^-149. No arithmetic: the unit's denormal mode has no say.
UR_PANO_FN float rgbe_value(uint32_t m, uint32_t e)
{
    if (m == 0u || e == 0u) return 0.0f;
    const uint32_t p = 31u - (uint32_t)__builtin_clz(m);
    const int32_t biased = (int32_t)(p + e) - 9;
    const uint32_t word = biased >= 1 ? ((uint32_t)biased << 23) | ((m << (23u - p)) & 0x7FFFFFu) : m << (e + 13u);
    float v;
    __builtin_memcpy(&v, &word, 4);
    return v;
}

// ---- atan2: |error| <= 2^-6 * 2 pi / 16384 rad against float64 (DESIGN.md 3.21 has the measured value). With a = min(|x|, |y|) / max(|x|, |y|)
// in [0, 1]: above tan(pi / 8) the angle is pi / 4 + atan((a - 1) / (a + 1)); atan(r) on |r| <= tan(pi / 8) is r P(r^2), P of degree 4
// (a weighted least-squares fit at Chebyshev nodes, within 6e-9 of atan in float64); then the octant, the half plane and y's sign.
// atan2(0, 0) = 0 whatever the signs; atan2(+-0, negative) = +-pi.
UR_PANO_FN float atan2_rule(float y, float x)
{
    const float ax = fabsf(x), ay = fabsf(y);
    const float hi = ax > ay ? ax : ay, lo = ax > ay ? ay : ax;
    if (!(hi > 0.0f)) return 0.0f;
    const float a = lo / hi;
    const bool upper = a > 0.41421357f;
    const float r = upper ? (a - 1.0f) / (a + 1.0f) : a;
    const float s = r * r;
    float p = 0.07882428169250488f;
    p = p * s + -0.13817109167575836f;
    p = p * s + 0.19971036911010742f;
    p = p * s + -0.3333272635936737f;
    p = p * s + 1.0f;
    float angle = r * p;
    if (upper) angle = 0.78539816339744831f + angle;
    if (ay > ax) angle = 1.57079632679489662f - angle;
    if (x < 0.0f) angle = 3.14159265358979324f - angle;
    return copysignf(angle, y);
}

// ---- the tap
// The direction of (s, t) on a face, by the inverse of ur_cube::cube_face's mapping (not normalised: only its angles are used):
//   +X (1, -t, -s)  -X (-1, -t, s)  +Y (s, 1, t)  -Y (s, -1, -t)  +Z (s, -t, 1)  -Z (-s, -t, -1)
UR_PANO_FN void face_direction(uint32_t face, float s, float t, float (&d)[3])
{
    d[0] = face == 0u ? 1.0f : (face == 1u ? -1.0f : (face == 5u ? -s : s));
    d[1] = face == 2u ? 1.0f : (face == 3u ? -1.0f : -t);
    d[2] = face == 0u ? -s : (face == 1u ? s : (face == 2u ? t : (face == 3u ? -t : (face == 4u ? 1.0f : -1.0f))));
}

// Where a direction lies in the panorama: the centre column looks along +Z, u grows towards +X, row 0 is +Y
UR_PANO_FN void panorama_uv(const float (&d)[3], float& u, float& v)
{
    u = 0.5f + atan2_rule(d[0], d[2]) * 0.15915494309189535f;
    v = 0.5f - atan2_rule(d[1], sqrtf(d[0] * d[0] + d[2] * d[2])) * 0.31830988618379069f;
}

// One bilinear sample of the panorama at (u, v), per channel on the decoded values: top = a + fx (b - a), bottom likewise,
// top + fy (bottom - top). Columns wrap modulo W, rows clamp to [0, H - 1]: whatever u and v are, the four texels are inside the source.
UR_PANO_FN void panorama_sample(const Plan& p, const uint32_t* rgbe, float u, float v, float (&out)[3])
{
    const float px = u * (float)p.width - 0.5f, py = v * (float)p.height - 0.5f;
    const float x0 = floorf(px), y0 = floorf(py);
    const float fx = px - x0, fy = py - y0;
    const int32_t W = (int32_t)p.width, H = (int32_t)p.height;
    // (u and v are in [0, 1] but for their last bits: the clamps in front of the conversions are for a caller's own u and v)
    int32_t ix = (int32_t)(x0 < -2.0f ? -2.0f : (x0 > 32768.0f ? 32768.0f : x0)) % W;
    if (ix < 0) ix += W;
    const int32_t ix1 = ix + 1 == W ? 0 : ix + 1;
    const int32_t iy = (int32_t)(y0 < -2.0f ? -2.0f : (y0 > 32768.0f ? 32768.0f : y0));
    const int32_t r0 = iy < 0 ? 0 : (iy > H - 1 ? H - 1 : iy), r1 = iy + 1 < 0 ? 0 : (iy + 1 > H - 1 ? H - 1 : iy + 1);
    const uint32_t a = rgbe[(size_t)r0 * p.width + (uint32_t)ix], b = rgbe[(size_t)r0 * p.width + (uint32_t)ix1];
    const uint32_t c = rgbe[(size_t)r1 * p.width + (uint32_t)ix], d = rgbe[(size_t)r1 * p.width + (uint32_t)ix1];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t ch = 0u; ch < 3u; ++ch) {
        const uint32_t sh = 8u * ch;
        const float va = rgbe_value((a >> sh) & 255u, a >> 24), vb = rgbe_value((b >> sh) & 255u, b >> 24);
        const float vc = rgbe_value((c >> sh) & 255u, c >> 24), vd = rgbe_value((d >> sh) & 255u, d >> 24);
        const float top = va + fx * (vb - va), bottom = vc + fx * (vd - vc);
        out[ch] = top + fy * (bottom - top);
    }
}

// Tap i = sy K + sx of output texel `texel` (of 6 E^2, face-major) added to acc
UR_PANO_FN void add_tap(const Plan& p, const uint32_t* rgbe, uint32_t texel, uint32_t i, float (&acc)[3])
{
    const uint32_t area = p.base * p.base, face = texel / area, rest = texel - face * area, y = rest / p.base, x = rest - y * p.base;
    const uint32_t sy = i / p.taps, sx = i - sy * p.taps;
    const float span = (float)(p.taps * p.base);
    const float s = (float)(2u * (x * p.taps + sx) + 1u) / span - 1.0f, t = (float)(2u * (y * p.taps + sy) + 1u) / span - 1.0f;
    float d[3], u, v, rgb[3];
    face_direction(face, s, t, d);
    panorama_uv(d, u, v);
    panorama_sample(p, rgbe, u, v, rgb);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int c = 0; c < 3; ++c) acc[c] = acc[c] + rgb[c];
}

// The texel a sum becomes: times 1 / K^2, at most the largest finite half, one rounding (in integers: cube_sample.h says why)
UR_PANO_FN uint64_t finish(const float (&sum)[3], float inv_taps2)
{
    uint64_t v = kAlphaOne;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int c = 0; c < 3; ++c) {
        const float mean = sum[c] * inv_taps2;
        v |= (uint64_t)ur_cube::half_bits(mean < kHalfMax ? mean : kHalfMax) << (16 * c);
    }
    return v;
}

// The rule, serial: output texel `texel`, the 64 lanes one after the other.
inline void texel_item(const Plan& p, const uint32_t* rgbe, uint64_t* dst, uint32_t texel)
{
    float lane[kLanes][3];
    const uint32_t taps2 = p.taps * p.taps;
    for (uint32_t j = 0u; j < kLanes; ++j) {
        lane[j][0] = lane[j][1] = lane[j][2] = 0.0f;
        for (uint32_t i = j; i < taps2; i += kLanes) add_tap(p, rgbe, texel, i, lane[j]);
    }
    for (uint32_t stride = kLanes / 2u; stride != 0u; stride >>= 1)
        for (uint32_t j = 0u; j < stride; ++j)
            for (int c = 0; c < 3; ++c) lane[j][c] = lane[j][c] + lane[j + stride][c];
    dst[texel] = finish(lane[0], p.inv_taps2);
}

// Where lane `lane` of wave `wave` works in the kernel's shape: its texel (>= p.texels: none) and its first tap
UR_PANO_FN void lane_place(const Plan& p, uint32_t wave, uint32_t lane, uint32_t& texel, uint32_t& tap)
{
    const bool packed = p.wave_texels > 1u;
    texel = wave * p.wave_texels + (packed ? lane >> p.taps2_log2 : 0u);
    tap = packed ? lane & ((1u << p.taps2_log2) - 1u) : lane;
}

// The kernel's wave, serial: wave_texels texels side by side, a lane's taps, the tree's strides below K^2 with every lane reading the
// lane `stride` above it (a lane past the wave's end reads its own value, as the shuffle gives it), the first lane of a texel storing it.
inline void wave_item(const Plan& p, const uint32_t* rgbe, uint64_t* dst, uint32_t wave)
{
    float sum[kLanes][3], next[kLanes][3];
    uint32_t texel[kLanes], tap[kLanes];
    const uint32_t taps2 = p.taps * p.taps;
    for (uint32_t l = 0u; l < kLanes; ++l) {
        lane_place(p, wave, l, texel[l], tap[l]);
        sum[l][0] = sum[l][1] = sum[l][2] = 0.0f;
        if (texel[l] < p.texels)
            for (uint32_t i = tap[l]; i < taps2; i += kLanes) add_tap(p, rgbe, texel[l], i, sum[l]);
    }
    for (uint32_t stride = kLanes / 2u; stride != 0u; stride >>= 1) {
        if (stride >= taps2) continue;
        for (uint32_t l = 0u; l < kLanes; ++l)
            for (int c = 0; c < 3; ++c) next[l][c] = sum[l][c] + sum[l + stride < kLanes ? l + stride : l][c];
        for (uint32_t l = 0u; l < kLanes; ++l)
            for (int c = 0; c < 3; ++c) sum[l][c] = next[l][c];
    }
    for (uint32_t l = 0u; l < kLanes; ++l)
        if (texel[l] < p.texels && tap[l] == 0u) dst[texel[l]] = finish(sum[l], p.inv_taps2);
}

} // namespace ur_pano
