// The staged environment cube's sampler as host and device code: the face choice, the 2 x 2 tap rule and the two-level blend that
// csrc/forward_resolve.hip (cube_face, cube_taps, cube_filter, cube_level_*) and the Lighting kernels run, over the bordered faces of
// csrc/lighting_plan.h - no edge logic, a face's one-texel ring holds its seamless neighbours. Plain inline functions with no HIP
// intrinsic, uncontracted fp32 with IEEE divides under build.py's EXACT flags; the environment prefilter (csrc/env_prefilter_rule.h,
// DESIGN.md section 3.20) samples through it on the device and on the host. Texels are 64-bit words (R | G << 16 | B << 32 | A << 48).
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#include "bc6h_decode.h" // UR_BC6H_FN

#define UR_CUBE_FN UR_BC6H_FN

namespace ur_cube {

constexpr float kFloatMax = 3.402823466e+38f;

// fp16 bits to fp32, exact
UR_CUBE_FN float half_value(uint32_t bits)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (float)__builtin_bit_cast(_Float16, (unsigned short)bits);
#else
    const uint32_t sign = (bits & 0x8000u) << 16, e = (bits >> 10) & 31u, m = bits & 0x3FFu;
    if (e == 0u) { // zero or subnormal: m * 2^-24
        const float v = (float)m * 5.9604644775390625e-8f;
        return sign ? -v : v;
    }
    const uint32_t word = sign | (e == 31u ? 0x7F800000u : (e + 112u) << 23) | (m << 13);
    float v;
    __builtin_memcpy(&v, &word, 4);
    return v;
#endif
}

// fp32 to fp16 bits, round to nearest even; at and above 65520 infinity; a NaN keeps its top payload bits. In integers on the device too:
// a cast to _Float16 there lets the compiler fuse a multiply in front of it into one v_fma_mixlo_f16, which rounds the exact product once
// where the rule rounds the fp32 product (seen on gfx950: one fp16 ulp in about one value of 10^4).
UR_CUBE_FN uint32_t half_bits(float v)
{
    uint32_t word;
    __builtin_memcpy(&word, &v, 4);
    const uint32_t sign = (word >> 16) & 0x8000u;
    uint32_t a = word & 0x7FFFFFFFu;
    if (a > 0x7F800000u) return sign | 0x7E00u | ((a >> 13) & 0x3FFu);
    if (a >= 0x477FF000u) return sign | 0x7C00u;
    if (a < 0x38800000u) { // below 2^-14: a subnormal half. In [0.5, 1) a float's ulp is 2^-24, the subnormal's step: the add rounds
        float f;
        __builtin_memcpy(&f, &a, 4);
        f += 0.5f;
        __builtin_memcpy(&a, &f, 4);
        return sign | (a - 0x3F000000u);
    }
    a += 0xFFFu + ((a >> 13) & 1u);
    return sign | ((a - 0x38000000u) >> 13);
}

UR_CUBE_FN float mix2(float a, float b, float t) { return a + t * (b - a); }
UR_CUBE_FN bool finite(float x) { return fabsf(x) <= kFloatMax; }

// D3D cube addressing (+X, -X, +Y, -Y, +Z, -Z; ties z > y > x): u = (sc / |ma| + 1) / 2
UR_CUBE_FN void cube_face(const float (&d)[3], uint32_t& face, float& u, float& v)
{
    const float ax = fabsf(d[0]), ay = fabsf(d[1]), az = fabsf(d[2]);
    const bool zmaj = az >= ax && az >= ay, ymaj = !zmaj && ay >= ax;
    const float comp = zmaj ? d[2] : (ymaj ? d[1] : d[0]);
    face = (zmaj ? 4u : (ymaj ? 2u : 0u)) + (comp < 0.0f ? 1u : 0u);
    const float ma = fabsf(comp);
    const float sc = face == 0u ? -d[2] : (face == 1u ? d[2] : (face == 5u ? -d[0] : d[0]));
    const float tc = face == 2u ? d[2] : (face == 3u ? -d[2] : -d[1]);
    u = (sc / ma + 1.0f) * 0.5f;
    v = (tc / ma + 1.0f) * 0.5f;
}

// The 2 x 2 taps of one bilinear sample of a level of edge N whose bordered faces start `offset` texels into `env`, and the weights
struct Taps { uint64_t t00, t10, t01, t11; float fx, fy; bool ok; };

UR_CUBE_FN Taps cube_taps(const uint64_t* env, uint32_t offset, uint32_t N, uint32_t face, float u, float v)
{
    Taps t;
    t.ok = finite(u) && finite(v);
    const float x = (t.ok ? u : 0.5f) * (float)N - 0.5f, y = (t.ok ? v : 0.5f) * (float)N - 0.5f;
    const float x0 = floorf(x), y0 = floorf(y);
    t.fx = x - x0;
    t.fy = y - y0;
    const int ix = (int)x0 + 1, iy = (int)y0 + 1, n = (int)N;
    const uint32_t i0 = (uint32_t)(ix < 0 ? 0 : (ix > n ? n : ix)), j0 = (uint32_t)(iy < 0 ? 0 : (iy > n ? n : iy)), E = N + 2u;
    const uint64_t* at = env + offset + (size_t)((face * E + j0) * E + i0);
    t.t00 = at[0]; t.t10 = at[1]; t.t01 = at[E]; t.t11 = at[E + 1u];
    return t;
}

UR_CUBE_FN void cube_filter(const Taps& t, float (&out)[3])
{
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int c = 0; c < 3; ++c) {
        const uint32_t sh = 16u * (uint32_t)c;
        const float a = half_value((uint32_t)(t.t00 >> sh) & 0xFFFFu), b = half_value((uint32_t)(t.t10 >> sh) & 0xFFFFu);
        const float d = half_value((uint32_t)(t.t01 >> sh) & 0xFFFFu), e = half_value((uint32_t)(t.t11 >> sh) & 0xFFFFu);
        const float value = mix2(mix2(a, b, t.fx), mix2(d, e, t.fx), t.fy);
        out[c] = t.ok ? value : __builtin_nanf("");
    }
}

// Where level m's bordered faces start in the staged cube of a power-of-two base with m <= log2(base), in texels: ur::CubeLayout::bordered
// in closed form. 6 * sum over j < m of (n_j + 2)^2 with n_j = base >> j: sum n_j^2 = 4 (base^2 - n_m^2) / 3, sum n_j = 2 (base - n_m).
UR_CUBE_FN uint32_t bordered_start(uint32_t base, uint32_t m)
{
    const uint32_t n = base >> m;
    return 8u * (base * base - n * n) + 48u * (base - n) + 24u * m;
}

// TextureCube.SampleLevel over the full chain (mips = log2(base) + 1) of a power-of-two cube of at most 2048: the level clamped to
// [0, mips - 1]; the upper level's taps are loaded whatever the fraction is, and blended in only when it is not zero.
UR_CUBE_FN void cube_sample_level(const uint64_t* env, uint32_t base, uint32_t mips, const float (&d)[3], float level, float (&out)[3])
{
    uint32_t face;
    float u, v;
    cube_face(d, face, u, v);
    const float top = (float)(mips - 1u);
    const float lv = level < 0.0f ? 0.0f : (level > top ? top : level);
    const uint32_t m0 = lv != lv ? 0u : (uint32_t)lv, m1 = m0 + 1u < mips - 1u ? m0 + 1u : mips - 1u;
    const float fl = lv - (float)m0;
    const Taps lo = cube_taps(env, bordered_start(base, m0), base >> m0, face, u, v), hi = cube_taps(env, bordered_start(base, m1), base >> m1, face, u, v);
    float a[3], b[3];
    cube_filter(lo, a);
    cube_filter(hi, b);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int c = 0; c < 3; ++c) out[c] = fl != 0.0f ? mix2(a[c], b[c], fl) : a[c];
}

} // namespace ur_cube
