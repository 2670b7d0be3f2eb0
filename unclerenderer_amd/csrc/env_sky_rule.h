// The sky capture (include/ur_env_sky.h): the procedural sky of SkyAtmosphere.hlsl:60-94 becomes the top level of
// an HDR cube, six square RGBA16F faces of a power-of-two edge E, face-major, alpha 1.0: exactly ur_env_prefilter's source and
// ur_env_panorama's output. This file is the rule as plain inline functions with no HIP intrinsic: the kernel of csrc/env_sky.hip calls
// them per lane, the serial host build (csrc/env_sky_host.cpp) and tests/cpp/env_sky_main.cpp call the same functions. fp32,
// uncontracted, IEEE divide and square root (build.py's EXACT flags); no libm function on the device: the shader's two exponentials and
// the sun's normalisation depend on the constants alone, so the host folds them in float64 (fold below), each rounded once to fp32.
//   fold     sun = LightDirection / |LightDirection|; h = max(0, CameraPosition.y);
//            scatter = rayleighColor * exp(-h / 8000) * 3 / (16 * 3.14159265); mie = LightColor * exp(-h / 1200) * 0.8 * (1 - 0.76^2) /
//            (4 * 3.14159265); attenuation = saturate(exp(-max(0, 1 - sun.y) * 2)). The shader's literals are fp32 values, widened exactly.
//   tap      sub-sample (sx, sy) of K x K of output texel (x, y): s = (2 (x K + sx) + 1) / (K E) - 1, t likewise (section 3.21's grid), the
//            direction by section 3.20's face table, d = direction / sqrt((dx^2 + dy^2) + dz^2), then ApplyAtmosphere in the order of
//            sky_value below: pow(x, 3) is (x x) x, pow(x, 1.5) is x sqrt(x) in front of the max(., 1e-3).
//   sum      section 3.20's order: tap i = sy K + sx; lane j of 64 starts at +0 and adds taps j, j + 64, ... ascending, a tree over the
//            lanes by strides 32 .. 1 follows, lane 0 times 1 / K^2, min(., 65504), one rounding to fp16.
// No tap and no sum of taps is -0 (the base sky is at least 0.05; x + (-x) is +0), so adding an idle lane's +0 changes nothing: a wave may
// hold 64 / K^2 texels when K^2 < 64 and run only the strides below K^2 (wave_item below, the kernel's shape, section 3.21's). The bytes
// are texel_item's.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "cube_sample.h" // ur_cube::half_bits

#define UR_SKY_FN UR_CUBE_FN

namespace ur_sky {

constexpr uint32_t kMaxBase = 2048u, kMaxTaps = 16u;
constexpr uint32_t kLanes = 64u; // the lanes a texel's taps are dealt to, whatever runs them
constexpr uint64_t kAlphaOne = 0x3C00ull << 48;
constexpr float kHalfMax = 65504.0f;

UR_SKY_FN bool power_of_two(uint32_t v) { return v != 0u && (v & (v - 1u)) == 0u; }

// The folded values: ten floats, the layout ur_host_env_sky_params returns
struct Params {
    float sun[3];      // the normalised LightDirection
    float scatter[3];  // rayleighColor * rayleighDensity * 3 / (16 pi)
    float mie[3];      // LightColor * mieDensity * 0.8 * (1 - g^2) / (4 pi)
    float attenuation; // saturate(exp(-max(0, 1 - sun.y) * 2))
};

// The refusals of ur_env_sky, ur_host_env_sky and ur_host_env_sky_params from the three vectors alone. Returns true (and the text).
inline bool refuse_constants(const char* who, const float* camera, const float* light_dir, const float* light_color, char* text, size_t text_size)
{
    for (int c = 0; c < 3; ++c)
        if (!ur_cube::finite(light_dir[c]) || !ur_cube::finite(light_color[c])) { snprintf(text, text_size, "%s: a LightDirection or LightColor that is not finite", who); return true; }
    if (!ur_cube::finite(camera[1])) { snprintf(text, text_size, "%s: a CameraPosition.y that is not finite", who); return true; }
    if (light_dir[0] == 0.0f && light_dir[1] == 0.0f && light_dir[2] == 0.0f) { snprintf(text, text_size, "%s: a LightDirection of length zero", who); return true; }
    return false;
}

// The refusals of ur_env_sky and ur_host_env_sky but for the constants', from the arguments alone.
inline bool refuse(const char* who, uint32_t base, uint32_t taps, const void* dst, size_t dst_bytes, char* text, size_t text_size)
{
    if (!dst) { snprintf(text, text_size, "%s: null destination", who); return true; }
    if (!power_of_two(base) || base > kMaxBase) { snprintf(text, text_size, "%s: base size %u (a power of two, 1..%u)", who, base, kMaxBase); return true; }
    if (!power_of_two(taps) || taps > kMaxTaps) { snprintf(text, text_size, "%s: %u taps a side (a power of two, 1..%u)", who, taps, kMaxTaps); return true; }
    const size_t dst_need = 48u * (size_t)base * base;
    if (dst_bytes != dst_need) { snprintf(text, text_size, "%s: %zu destination bytes, %zu expected (six faces of %u x %u RGBA16F texels)", who, dst_bytes, dst_need, base, base); return true; }
    if (reinterpret_cast<uintptr_t>(dst) % 16u != 0u) { snprintf(text, text_size, "%s: destination not 16-byte aligned", who); return true; }
    return false;
}

// fold: float64, every value rounded once (host only: exp and sqrt in double)
inline Params fold(const float* camera, const float* light_dir, const float* light_color)
{
    const double pi = (double)3.14159265f, g = (double)0.76f;
    const double lx = light_dir[0], ly = light_dir[1], lz = light_dir[2];
    // (fp32 components squared and added in double neither overflow nor vanish)
    const double len = sqrt(lx * lx + ly * ly + lz * lz);
    const double sun[3] = {lx / len, ly / len, lz / len};
    const double h = (double)camera[1] > 0.0 ? (double)camera[1] : 0.0;
    const double rayleigh = exp(-h / 8000.0), mie = exp(-h / 1200.0);
    const double colour[3] = {(double)0.650f, (double)0.570f, (double)0.475f};
    Params p;
    for (int c = 0; c < 3; ++c) {
        p.sun[c] = (float)sun[c];
        p.scatter[c] = (float)(colour[c] * rayleigh * (3.0 / (16.0 * pi)));
        p.mie[c] = (float)((double)light_color[c] * mie * ((double)0.8f * ((1.0 - g * g) / (4.0 * pi))));
    }
    const double up = 1.0 - sun[1] > 0.0 ? 1.0 - sun[1] : 0.0;
    const double a = exp(-up * 2.0);
    p.attenuation = (float)(a < 0.0 ? 0.0 : (a > 1.0 ? 1.0 : a));
    return p;
}

// ---- the plan
struct Plan {
    Params sky;
    uint32_t base, taps;
    uint32_t taps2_log2;  // log2(taps^2): 0, 2, 4, 6, 8
    uint32_t texels;      // 6 base^2
    uint32_t wave_texels; // the texels a wave holds: 64 / taps^2, at least 1
    uint32_t waves;
    float inv_taps2;      // 1 / taps^2, a power of two
};

inline Plan make_plan(const Params& sky, uint32_t base, uint32_t taps)
{
    Plan p{};
    p.sky = sky;
    p.base = base; p.taps = taps;
    while ((1u << p.taps2_log2) < taps * taps) ++p.taps2_log2;
    p.texels = 6u * base * base;
    p.wave_texels = taps * taps < kLanes ? kLanes / (taps * taps) : 1u;
    p.waves = (p.texels + p.wave_texels - 1u) / p.wave_texels;
    p.inv_taps2 = 1.0f / (float)(taps * taps);
    return p;
}

// ---- the tap
// The direction of (s, t) on a face, by the inverse of ur_cube::cube_face's mapping:
//   +X (1, -t, -s)  -X (-1, -t, s)  +Y (s, 1, t)  -Y (s, -1, -t)  +Z (s, -t, 1)  -Z (-s, -t, -1)
UR_SKY_FN void face_direction(uint32_t face, float s, float t, float (&d)[3])
{
    d[0] = face == 0u ? 1.0f : (face == 1u ? -1.0f : (face == 5u ? -s : s));
    d[1] = face == 2u ? 1.0f : (face == 3u ? -1.0f : -t);
    d[2] = face == 0u ? -s : (face == 1u ? s : (face == 2u ? t : (face == 3u ? -t : (face == 4u ? 1.0f : -1.0f))));
}

UR_SKY_FN float saturate(float x) { return x > 0.0f ? (x < 1.0f ? x : 1.0f) : 0.0f; }

// ApplyAtmosphere (SkyAtmosphere.hlsl:60-94) for the unit direction d, over the folded values: the operation order is the rule
UR_SKY_FN void sky_value(const Params& k, const float (&d)[3], float (&out)[3])
{
    const float h = 1.0f - saturate(d[1] * 0.5f + 0.5f);
    const float falloff = saturate((h * h) * h); // pow(., 3)
    const float cos_sun = (d[0] * k.sun[0] + d[1] * k.sun[1]) + d[2] * k.sun[2];
    const float rayleigh = 1.0f + cos_sun * cos_sun;
    const float g = 0.76f;
    const float mb = (1.0f + g * g) - (2.0f * g) * cos_sun;
    const float denom = mb * sqrtf(mb); // pow(., 1.5); mb >= (1 - g)^2 but for cos_sun's last bit
    const float mie = 1.0f / (denom > 1e-3f ? denom : 1e-3f);
    const float zenith[3] = {0.05f, 0.12f, 0.22f}, horizon[3] = {0.52f, 0.68f, 0.86f};
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int c = 0; c < 3; ++c) {
        const float base = zenith[c] + falloff * (horizon[c] - zenith[c]);
        out[c] = base + (k.scatter[c] * rayleigh + k.mie[c] * mie) * k.attenuation;
    }
}

// Tap i = sy K + sx of output texel `texel` (of 6 E^2, face-major) added to acc
UR_SKY_FN void add_tap(const Plan& p, uint32_t texel, uint32_t i, float (&acc)[3])
{
    const uint32_t area = p.base * p.base, face = texel / area, rest = texel - face * area, y = rest / p.base, x = rest - y * p.base;
    const uint32_t sy = i / p.taps, sx = i - sy * p.taps;
    const float span = (float)(p.taps * p.base);
    const float s = (float)(2u * (x * p.taps + sx) + 1u) / span - 1.0f, t = (float)(2u * (y * p.taps + sy) + 1u) / span - 1.0f;
    float d[3], rgb[3];
    face_direction(face, s, t, d);
    const float len = sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    d[0] = d[0] / len; d[1] = d[1] / len; d[2] = d[2] / len;
    sky_value(p.sky, d, rgb);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int c = 0; c < 3; ++c) acc[c] = acc[c] + rgb[c];
}

// The texel a sum becomes: times 1 / K^2, at most the largest finite half, one rounding (in integers: cube_sample.h says why)
UR_SKY_FN uint64_t finish(const float (&sum)[3], float inv_taps2)
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
inline void texel_item(const Plan& p, uint64_t* dst, uint32_t texel)
{
    float lane[kLanes][3];
    const uint32_t taps2 = p.taps * p.taps;
    for (uint32_t j = 0u; j < kLanes; ++j) {
        lane[j][0] = lane[j][1] = lane[j][2] = 0.0f;
        for (uint32_t i = j; i < taps2; i += kLanes) add_tap(p, texel, i, lane[j]);
    }
    for (uint32_t stride = kLanes / 2u; stride != 0u; stride >>= 1)
        for (uint32_t j = 0u; j < stride; ++j)
            for (int c = 0; c < 3; ++c) lane[j][c] = lane[j][c] + lane[j + stride][c];
    dst[texel] = finish(lane[0], p.inv_taps2);
}

// Where lane `lane` of wave `wave` works in the kernel's shape: its texel (>= p.texels: none) and its first tap
UR_SKY_FN void lane_place(const Plan& p, uint32_t wave, uint32_t lane, uint32_t& texel, uint32_t& tap)
{
    const bool packed = p.wave_texels > 1u;
    texel = wave * p.wave_texels + (packed ? lane >> p.taps2_log2 : 0u);
    tap = packed ? lane & ((1u << p.taps2_log2) - 1u) : lane;
}

// The kernel's wave, serial: wave_texels texels side by side, a lane's taps, the tree's strides below K^2 with every lane reading the
// lane `stride` above it (a lane past the wave's end reads its own value, as the shuffle gives it), the first lane of a texel storing it.
inline void wave_item(const Plan& p, uint64_t* dst, uint32_t wave)
{
    float sum[kLanes][3], next[kLanes][3];
    uint32_t texel[kLanes], tap[kLanes];
    const uint32_t taps2 = p.taps * p.taps;
    for (uint32_t l = 0u; l < kLanes; ++l) {
        lane_place(p, wave, l, texel[l], tap[l]);
        sum[l][0] = sum[l][1] = sum[l][2] = 0.0f;
        if (texel[l] < p.texels)
            for (uint32_t i = tap[l]; i < taps2; i += kLanes) add_tap(p, texel[l], i, sum[l]);
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

} // namespace ur_sky
