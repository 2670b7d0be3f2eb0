// The environment cube build (include/ur_env_cube.h): a DDS cube payload - BC6H blocks or RGBA16F texels, six
// faces, face-major with mips inner - becomes the staged cube of csrc/lighting_plan.h, the bytes ur_stage_env_cube writes. This file is
// the rule as work items, plain inline functions with no HIP intrinsic: the three kernels of csrc/env_cube_build.hip call one function
// each per lane, and tests/cpp/env_cube_main.cpp calls the same functions item by item on the host, under ASan, before any device run.
//   decode  item = one texel row of one block column of one level of one face: up to four texels, straight into the interior of the
//           level's bordered face. Texels past the level's edge (levels of edge 1, 2, 3, 5, 6 ...) are not written.
//   border  item = one texel of a bordered face's one-texel ring: a copy of the interior texel border_source() names.
//   pairs   item = one 12-byte row-pair entry, from the bordered section.
// border_source is ur_stage_env_cube's resolve_border (csrc/env_cube_stage.cpp) in integers. With s = (2 i + 1 - N) / N the coordinates
// times N are integers; the overshoot |s| - 1 is exactly 1 / N, so the folded point's major coordinate times N is +-(N - 1); and the
// texel of a folded coordinate A / N is floor((A + N) / 2) with A + N always odd: A is +-(N - 1) or +-(2 j + 1 - N). The floor never
// sits on an edge, which is why the double arithmetic of resolve_border and this agree (held for every edge 1..64 and 256 by the tests).
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "bc6h_decode.h"
#include "lighting_plan.h"
#include "ur_checks.h" // ur::overlaps (host only, inline)

#define UR_ENVC_FN UR_BC6H_FN

namespace ur_envc {

constexpr uint32_t kRGBA16F = 10u, kUF16 = 95u, kSF16 = 96u; // DXGI_FORMAT_R16G16B16A16_FLOAT, BC6H_UF16, BC6H_SF16
constexpr uint32_t kMaxBase = 16384u;                        // every item count of such a cube is below 2^32
constexpr uint32_t kLevels = 16u;

UR_ENVC_FN bool is_format(uint32_t format) { return format == kRGBA16F || format == kUF16 || format == kSF16; }
UR_ENVC_FN bool is_bc6h(uint32_t format) { return format == kUF16 || format == kSF16; }
UR_ENVC_FN uint32_t level_size(uint32_t base, uint32_t m) { return (base >> m) > 1u ? (base >> m) : 1u; }
UR_ENVC_FN uint32_t blocks_across(uint32_t n) { return (n + 3u) >> 2; }

// bytes of the payload; 0 for what ur::cube_layout refuses and for an unknown format
inline size_t source_bytes(uint32_t format, uint32_t base, uint32_t mips)
{
    if (!is_format(format) || base == 0u || mips == 0u || mips > kLevels) return 0u;
    size_t bytes = 0u;
    for (uint32_t m = 0u; m < mips; ++m) {
        const size_t n = level_size(base, m), across = blocks_across((uint32_t)n);
        bytes += is_bc6h(format) ? across * across * 16u : n * n * 8u;
    }
    return 6u * bytes;
}

// The refusals of ur_env_cube_build and ur_host_env_cube_build, from the arguments alone. Returns true (and the text) on a refusal.
inline bool refuse(const char* who, const void* src, size_t src_bytes, uint32_t format, uint32_t base, uint32_t mips, const void* dst, size_t dst_texels,
                   const void* info, char* text, size_t text_size)
{
    if (!src || !dst) { snprintf(text, text_size, "%s: null source or destination", who); return true; }
    if (!is_format(format)) { snprintf(text, text_size, "%s: source format %u (10, 95, 96)", who, format); return true; }
    const ur::CubeLayout L = ur::cube_layout(base, mips);
    if (L.mips == 0u || base > kMaxBase) { snprintf(text, text_size, "%s: no cube: base size %u, %u mips (sizes 1..%u, mips 1..16)", who, base, mips, kMaxBase); return true; }
    const size_t need = source_bytes(format, base, mips);
    if (src_bytes != need) { snprintf(text, text_size, "%s: %zu source bytes, %zu expected (ur_env_cube_source_bytes)", who, src_bytes, need); return true; }
    if (dst_texels != (size_t)L.texels) { snprintf(text, text_size, "%s: %zu destination texels, %zu expected (ur_env_cube_texels)", who, dst_texels, (size_t)L.texels); return true; }
    if (reinterpret_cast<uintptr_t>(src) % 16u != 0u) { snprintf(text, text_size, "%s: source not 16-byte aligned", who); return true; }
    if (reinterpret_cast<uintptr_t>(dst) % 16u != 0u) { snprintf(text, text_size, "%s: destination not 16-byte aligned", who); return true; }
    if (reinterpret_cast<uintptr_t>(info) % 4u != 0u) { snprintf(text, text_size, "%s: info not 4-byte aligned", who); return true; }
    const size_t dst_bytes = (size_t)L.bytes;
    if (ur::overlaps(src, src_bytes, dst, dst_bytes)) { snprintf(text, text_size, "%s: source and destination overlap", who); return true; }
    if (info && ur::overlaps(src, src_bytes, info, 4u)) { snprintf(text, text_size, "%s: source and info overlap", who); return true; }
    if (info && ur::overlaps(dst, dst_bytes, info, 4u)) { snprintf(text, text_size, "%s: destination and info overlap", who); return true; }
    return false;
}

// ---- the plan: where every level's items, source and destination start. Entries behind the chain's end hold the per-face totals, so
// the search below never selects them.
struct Plan {
    uint32_t base, mips, format;
    uint32_t face_source;                     // source units a face: 16-byte blocks (BC6H) or 8-byte texels (RGBA16F)
    uint32_t decode_face, border_face, pair_face; // items a face
    uint32_t total_blocks;                    // BC6H blocks of the whole payload (0: RGBA16F)
    uint32_t source_start[kLevels];           // source units of a face in front of level m
    uint32_t decode_start[kLevels], border_start[kLevels], pair_start[kLevels]; // items of a face in front of level m
    uint64_t bordered[kLevels];               // ur::CubeLayout::bordered, in texels
    uint64_t pairs[kLevels];                  // ur::CubeLayout::pairs, in bytes
};

inline Plan make_plan(uint32_t format, uint32_t base, uint32_t mips)
{
    Plan p{};
    const ur::CubeLayout L = ur::cube_layout(base, mips);
    p.base = base; p.mips = mips; p.format = format;
    uint32_t source = 0u, decode = 0u, border = 0u, pair = 0u;
    for (uint32_t m = 0u; m < kLevels; ++m) {
        p.source_start[m] = source; p.decode_start[m] = decode; p.border_start[m] = border; p.pair_start[m] = pair;
        if (m >= mips) continue;
        const uint32_t n = level_size(base, m), across = blocks_across(n), e = n + 2u;
        source += is_bc6h(format) ? across * across : n * n;
        decode += n * across;
        border += 4u * (n + 1u);
        pair += (e - 1u) * e;
        p.bordered[m] = L.bordered[m];
        p.pairs[m] = L.pairs[m];
    }
    p.face_source = source; p.decode_face = decode; p.border_face = border; p.pair_face = pair;
    p.total_blocks = is_bc6h(format) ? 6u * source : 0u;
    return p;
}

// the level of a face's item: the last m whose start is not above it (selects: no array under a run-time index)
UR_ENVC_FN uint32_t level_of(const uint32_t (&start)[kLevels], uint32_t item)
{
    uint32_t level = 0u;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t m = 1u; m < kLevels; ++m) level = item >= start[m] ? m : level;
    return level;
}
UR_ENVC_FN uint32_t at32(const uint32_t (&a)[kLevels], uint32_t level)
{
    uint32_t v = a[0];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t m = 1u; m < kLevels; ++m) v = level == m ? a[m] : v;
    return v;
}
UR_ENVC_FN uint64_t at64(const uint64_t (&a)[kLevels], uint32_t level)
{
    uint64_t v = a[0];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t m = 1u; m < kLevels; ++m) v = level == m ? a[m] : v;
    return v;
}

// ---- the border rule, in integers
struct Texel { int face, i, j; };

// Face addressing is D3D's (+X, -X, +Y, -Y, +Z, -Z): p[major] = ms, p[su] = us * s, p[sv] = vs * t with
//   +X (1, -t, -s)  -X (-1, -t, s)  +Y (s, 1, t)  -Y (s, -1, -t)  +Z (s, -t, 1)  -Z (-s, -t, -1)
UR_ENVC_FN int face_major(int f) { return f >> 1; }
UR_ENVC_FN int face_su(int f) { return f < 2 ? 2 : 0; }
UR_ENVC_FN int face_sv(int f) { return (f >> 1) == 1 ? 2 : 1; }
UR_ENVC_FN int face_ms(int f) { return (f & 1) ? -1 : 1; }
UR_ENVC_FN int face_us(int f) { return ((0x21 >> f) & 1) ? -1 : 1; } // negative on +X and -Z
UR_ENVC_FN int face_vs(int f) { return ((0x3B >> f) & 1) ? -1 : 1; } // positive on +Y alone
UR_ENVC_FN int axis_of(int p0, int p1, int p2, int axis) { return axis == 0 ? p0 : (axis == 1 ? p1 : p2); }

// The interior texel a texel of face `face`'s border ring copies; (i, j) with i or j equal to -1 or N. A corner clamps j first.
UR_ENVC_FN Texel border_source(int N, int face, int i, int j)
{
    const bool iOut = i < 0 || i >= N, jOut = j < 0 || j >= N;
    if (iOut && jOut) j = j < 0 ? 0 : N - 1;
    const int a = 2 * i + 1 - N, b = 2 * j + 1 - N; // s N and t N
    const int major = face_major(face), su = face_su(face);
    const int pm = face_ms(face) * (N - 1), pu = face_us(face) * a, pv = face_vs(face) * b; // the folded point times N, but for the axis it folds over
    const int p0 = major == 0 ? pm : (su == 0 ? pu : pv), p1 = major == 1 ? pm : (su == 1 ? pu : pv), p2 = major == 2 ? pm : (su == 2 ? pu : pv);
    const int oa = iOut ? su : face_sv(face);
    const int nf = oa * 2 + (axis_of(p0, p1, p2, oa) > 0 ? 0 : 1);
    const int A = axis_of(p0, p1, p2, face_su(nf)) * face_us(nf), B = axis_of(p0, p1, p2, face_sv(nf)) * face_vs(nf);
    int oi = (A + N) >> 1, oj = (B + N) >> 1; // A + N and B + N are odd and positive
    oi = oi < 0 ? 0 : (oi >= N ? N - 1 : oi);
    oj = oj < 0 ? 0 : (oj >= N ? N - 1 : oj);
    return Texel{nf, oi, oj};
}

// ---- the items. `dst` is the staged cube as 64-bit texels (R | G << 16 | B << 32 | A << 48).
// decode: item < 6 * decode_face. is_signed / bc6h are the plan's format, as constants where the caller has them.
UR_ENVC_FN void decode_item(const Plan& p, const void* src, uint64_t* dst, uint32_t item, bool bc6h, bool is_signed, const ur_bc6h::Tables* tables)
{
    const uint32_t face = item / p.decode_face, rest = item - face * p.decode_face;
    const uint32_t m = level_of(p.decode_start, rest), j = rest - at32(p.decode_start, m);
    const uint32_t n = level_size(p.base, m), across = blocks_across(n), e = n + 2u;
    const uint32_t y = j / across, bx = j - y * across;
    const uint32_t inside = n - 4u * bx < 4u ? n - 4u * bx : 4u; // texels of this block row inside the level
    const size_t unit = (size_t)face * p.face_source + at32(p.source_start, m);
    uint64_t* out = dst + (at64(p.bordered, m) + ((uint64_t)face * e + y + 1u) * e + 4u * bx + 1u);
    if (bc6h) {
        const uint64_t* block = static_cast<const uint64_t*>(src) + 2u * (unit + (size_t)(y >> 2) * across + bx);
        const uint64_t lo = block[0], hi = block[1];
        ur_bc6h::Header h;
        const bool ok = ur_bc6h::decode_header(lo, hi, is_signed, h);
        const uint32_t first = 4u * (y & 3u);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (uint32_t k = 0u; k < 4u; ++k)
            if (k < inside) out[k] = ok ? ur_bc6h::texel(h, lo, hi, first + k, is_signed, tables) : ur_bc6h::kReservedTexel;
    } else {
        const uint64_t* row = static_cast<const uint64_t*>(src) + (unit + (size_t)y * n + 4u * bx);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (uint32_t k = 0u; k < 4u; ++k)
            if (k < inside) out[k] = row[k];
    }
}

// border: item < 6 * border_face. Reads interior texels only, writes ring texels only.
UR_ENVC_FN void border_item(const Plan& p, uint64_t* dst, uint32_t item)
{
    const uint32_t face = item / p.border_face, rest = item - face * p.border_face;
    const uint32_t m = level_of(p.border_start, rest), k = rest - at32(p.border_start, m);
    const int n = (int)level_size(p.base, m);
    const uint32_t side = k / (uint32_t)(n + 1), t = k - side * (uint32_t)(n + 1);
    // the ring, clockwise from its top-left corner: n + 1 texels a side
    const int i = side == 0u ? (int)t - 1 : (side == 1u ? n : (side == 2u ? n - (int)t : -1));
    const int j = side == 0u ? -1 : (side == 1u ? (int)t - 1 : (side == 2u ? n : n - (int)t));
    const Texel s = border_source(n, (int)face, i, j);
    const uint64_t e = (uint64_t)n + 2u;
    uint64_t* level = dst + at64(p.bordered, m);
    level[((uint64_t)face * e + (uint64_t)(j + 1)) * e + (uint64_t)(i + 1)] = level[((uint64_t)s.face * e + (uint64_t)(s.j + 1)) * e + (uint64_t)(s.i + 1)];
}

// pairs: item < 6 * pair_face. Entry (f, j, i) is {R G B of bordered texel (i, j), R G B of (i, j + 1)}: 12 bytes, three words.
UR_ENVC_FN void pair_item(const Plan& p, uint64_t* dst, uint32_t item)
{
    const uint32_t face = item / p.pair_face, rest = item - face * p.pair_face;
    const uint32_t m = level_of(p.pair_start, rest), k = rest - at32(p.pair_start, m);
    const uint32_t e = level_size(p.base, m) + 2u;
    const uint32_t j = k / e, i = k - j * e;
    const uint64_t* level = dst + at64(p.bordered, m);
    const uint64_t t0 = level[((uint64_t)face * e + j) * e + i], t1 = level[((uint64_t)face * e + j + 1u) * e + i];
    uint32_t* out = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(dst) + at64(p.pairs, m)) + 3u * (((uint64_t)face * (e - 1u) + j) * e + i);
    out[0] = (uint32_t)t0;
    out[1] = ((uint32_t)(t0 >> 32) & 0xFFFFu) | ((uint32_t)t1 << 16);
    out[2] = (uint32_t)(t1 >> 16);
}

} // namespace ur_envc
