// The source formats of the texture transcode (DESIGN.md section 3.15 is the rule, tests/texture_source_ref.py the restatement): BC2, BC4
// and BC7 beside the BC1 / BC3 / BC5 of csrc/bc_decode.h, whose functions this file calls and leaves as they are - the sampler's validity
// test (is_bc, block_bytes) does not learn the new codes. "The RGBA8 code word of texel n of this block" as plain inline functions with
// no HIP intrinsic: csrc/texture_transcode.hip (device) and csrc/bc_host.cpp (host, any C++ compiler) include this very file.
// BC7 needs tables under a run-time index - the mode's field widths, the partition rows, the anchors, the weights. They are one packed
// struct of 640 bytes passed by pointer: the host uses kWideTables itself, a kernel stages a copy in LDS once per workgroup. A local
// array under a run-time index would become scratch; every field of a block is fetched by its bit position instead.
#pragma once

#include "bc_decode.h"

namespace ur_bc {

constexpr uint32_t kBC2 = 74u, kBC2Srgb = 75u, kBC4 = 80u, kBC7 = 98u, kBC7Srgb = 99u; // DXGI_FORMAT_BC2_UNORM[_SRGB], BC4_UNORM, BC7_UNORM[_SRGB]

UR_BC_FN bool is_bc2(uint32_t format) { return format == kBC2 || format == kBC2Srgb; }
UR_BC_FN bool is_bc7(uint32_t format) { return format == kBC7 || format == kBC7Srgb; }
// the ten formats a chain can be transcoded from
UR_BC_FN bool is_source(uint32_t format) { return is_bc(format) || is_bc2(format) || format == kBC4 || is_bc7(format); }
UR_BC_FN uint32_t source_block_bytes(uint32_t format) { return is_bc(format) ? block_bytes(format) : (format == kBC4 ? 8u : (is_bc2(format) || is_bc7(format) ? 16u : 0u)); }
// does the RGBA8 chain of this source carry UR_TEXTURE_R8G8B8A8_UNORM_SRGB (29)?
UR_BC_FN bool source_is_srgb(uint32_t format) { return format == kBC1Srgb || format == kBC3Srgb || format == kBC2Srgb || format == kBC7Srgb; }
UR_BC_FN size_t source_chain_bytes(uint32_t format, uint32_t width, uint32_t height, uint32_t mips) { return chain_blocks(width, height, mips) * source_block_bytes(format); }
// texels of ur_texture2d's RGBA8 chain in front of level d = texels of a chain of d levels (4 bytes each)
UR_BC_FN uint64_t chain_texels(uint32_t width, uint32_t height, uint32_t d)
{
    uint64_t texels = 0u;
    for (uint32_t k = 0u; k < d; ++k) texels += (uint64_t)level_size(width, k) * level_size(height, k);
    return texels;
}

// ---- BC7's tables. A mode's fields in one word: subsets | partition bits << 2 | rotation bits << 5 | index-selection bits << 7 |
// colour bits << 8 | alpha bits << 11 | p-bit per endpoint << 15 | p-bit per subset << 16 | index bits << 17 | second index bits << 20.
constexpr uint32_t mode_word(uint32_t subsets, uint32_t pb, uint32_t rb, uint32_t isb, uint32_t cb, uint32_t ab, uint32_t epb, uint32_t spb, uint32_t ib, uint32_t ib2)
{
    return subsets | (pb << 2) | (rb << 5) | (isb << 7) | (cb << 8) | (ab << 11) | (epb << 15) | (spb << 16) | (ib << 17) | (ib2 << 20);
}
struct WideTables {
    uint32_t mode[8];
    uint32_t part3[64];  // three subsets: texel n's subset at bits 2n
    uint16_t part2[64];  // two subsets: texel n's subset at bit n
    uint8_t anchor2[64]; // two subsets: the anchor texel of subset 1
    uint8_t anchor3a[64], anchor3b[64]; // three subsets: the anchor texels of subset 1 and of subset 2
    uint8_t weights[32]; // 2-bit indices at 0, 3-bit at 4, 4-bit at 12; four bytes of padding
};
static_assert(sizeof(WideTables) == 640, "staged as 160 dwords");
// The rows and anchors are BPTC's public tables (Khronos Data Format Specification, BPTC; Microsoft, "BC7 Format"). Every entry is held by
// tests/golden/texture_source_pillow.npz: per partition, a mode-1 / mode-2 block with distinct constant endpoints per subset shows its
// row in Pillow's texels, and one with all index bits set shows its anchors as the texels that are not 255.
constexpr WideTables kWideTables = {
    {mode_word(3, 4, 0, 0, 4, 0, 1, 0, 3, 0), mode_word(2, 6, 0, 0, 6, 0, 0, 1, 3, 0), mode_word(3, 6, 0, 0, 5, 0, 0, 0, 2, 0), mode_word(2, 6, 0, 0, 7, 0, 1, 0, 2, 0),
     mode_word(1, 0, 2, 1, 5, 6, 0, 0, 2, 3), mode_word(1, 0, 2, 0, 7, 8, 0, 0, 2, 2), mode_word(1, 0, 0, 0, 7, 7, 1, 0, 4, 0), mode_word(2, 6, 0, 0, 5, 5, 1, 0, 2, 0)},
    {0xAA685050u, 0x6A5A5040u, 0x5A5A4200u, 0x5450A0A8u, 0xA5A50000u, 0xA0A05050u, 0x5555A0A0u, 0x5A5A5050u, 0xAA550000u, 0xAA555500u, 0xAAAA5500u,
     0x90909090u, 0x94949494u, 0xA4A4A4A4u, 0xA9A59450u, 0x2A0A4250u, 0xA5945040u, 0x0A425054u, 0xA5A5A500u, 0x55A0A0A0u, 0xA8A85454u, 0x6A6A4040u,
     0xA4A45000u, 0x1A1A0500u, 0x0050A4A4u, 0xAAA59090u, 0x14696914u, 0x69691400u, 0xA08585A0u, 0xAA821414u, 0x50A4A450u, 0x6A5A0200u, 0xA9A58000u,
     0x5090A0A8u, 0xA8A09050u, 0x24242424u, 0x00AA5500u, 0x24924924u, 0x24499224u, 0x50A50A50u, 0x500AA550u, 0xAAAA4444u, 0x66660000u, 0xA5A0A5A0u,
     0x50A050A0u, 0x69286928u, 0x44AAAA44u, 0x66666600u, 0xAA444444u, 0x54A854A8u, 0x95809580u, 0x96969600u, 0xA85454A8u, 0x80959580u, 0xAA141414u,
     0x96960000u, 0xAAAA1414u, 0xA05050A0u, 0xA0A5A5A0u, 0x96000000u, 0x40804080u, 0xA9A8A9A8u, 0xAAAAAA44u, 0x2A4A5254u},
    {0xCCCC, 0x8888, 0xEEEE, 0xECC8, 0xC880, 0xFEEC, 0xFEC8, 0xEC80, 0xC800, 0xFFEC, 0xFE80, 0xE800, 0xFFE8, 0xFF00, 0xFFF0, 0xF000,
     0xF710, 0x008E, 0x7100, 0x08CE, 0x008C, 0x7310, 0x3100, 0x8CCE, 0x088C, 0x3110, 0x6666, 0x366C, 0x17E8, 0x0FF0, 0x718E, 0x399C,
     0xAAAA, 0xF0F0, 0x5A5A, 0x33CC, 0x3C3C, 0x55AA, 0x9696, 0xA55A, 0x73CE, 0x13C8, 0x324C, 0x3BDC, 0x6996, 0xC33C, 0x9966, 0x0660,
     0x0272, 0x04E4, 0x4E40, 0x2720, 0xC936, 0x936C, 0x39C6, 0x639C, 0x9336, 0x9CC6, 0x817E, 0xE718, 0xCCF0, 0x0FCC, 0x7744, 0xEE22},
    {15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 2, 8, 2, 2, 8, 8, 15, 2, 8, 2, 2, 8, 8, 2, 2,
     15, 15, 6, 8, 2, 8, 15, 15, 2, 8, 2, 2, 2, 15, 15, 6, 6, 2, 6, 8, 15, 15, 2, 2, 15, 15, 15, 15, 15, 2, 2, 15},
    {3, 3, 15, 15, 8, 3, 15, 15, 8, 8, 6, 6, 6, 5, 3, 3, 3, 3, 8, 15, 3, 3, 6, 10, 5, 8, 8, 6, 8, 5, 15, 15,
     8, 15, 3, 5, 6, 10, 8, 15, 15, 3, 15, 5, 15, 15, 15, 15, 3, 15, 5, 5, 5, 8, 5, 10, 5, 10, 8, 13, 15, 12, 3, 3},
    {15, 8, 8, 3, 15, 15, 3, 8, 15, 15, 15, 15, 15, 15, 15, 8, 15, 8, 15, 3, 15, 8, 15, 8, 3, 15, 6, 10, 15, 15, 10, 8,
     15, 3, 15, 10, 10, 8, 9, 10, 6, 15, 8, 15, 3, 6, 6, 8, 15, 3, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 3, 15, 15, 8},
    {0, 21, 43, 64, 0, 9, 18, 27, 37, 46, 55, 64, 0, 4, 9, 13, 17, 21, 26, 30, 34, 38, 43, 47, 51, 55, 60, 64, 0, 0, 0, 0}};

// ---- `count` bits (0..16) of the 128-bit block from bit `pos` on, least significant first; pos + count <= 128
UR_BC_FN uint32_t block_bits(uint64_t lo, uint64_t hi, uint32_t pos, uint32_t count)
{
    const uint64_t v = pos >= 64u ? hi >> (pos - 64u) : (lo >> pos) | ((hi << 1) << (63u - pos));
    return (uint32_t)v & ((1u << count) - 1u);
}
// an endpoint of `b` bits (5..8, the p-bit included) to 8 bits
UR_BC_FN uint32_t expand_endpoint(uint32_t v, uint32_t b) { return ((v << (8u - b)) | (v >> (2u * b - 8u))) & 255u; }
UR_BC_FN uint32_t interpolate(uint32_t e0, uint32_t e1, uint32_t w) { return ((64u - w) * e0 + w * e1 + 32u) >> 6; }

// ---- BC7: the code word of texel n. The mode is the lowest set bit of byte 0; byte 0 == 0 is the reserved mode, (0, 0, 0, 0).
UR_BC_FN uint32_t bc7_word(uint64_t lo, uint64_t hi, uint32_t n, const WideTables* t)
{
    const uint32_t byte0 = (uint32_t)lo & 255u;
    if (byte0 == 0u) return 0u;
    const uint32_t low = byte0 & (0u - byte0); // the lowest set bit alone
    const uint32_t m = ((low & 0xAAu) != 0u ? 1u : 0u) | ((low & 0xCCu) != 0u ? 2u : 0u) | ((low & 0xF0u) != 0u ? 4u : 0u);
    const uint32_t mw = t->mode[m];
    const uint32_t subsets = mw & 3u, pb = (mw >> 2) & 7u, rb = (mw >> 5) & 3u, isb = (mw >> 7) & 1u, cb = (mw >> 8) & 7u, ab = (mw >> 11) & 15u;
    const uint32_t epb = (mw >> 15) & 1u, spb = (mw >> 16) & 1u, ib = (mw >> 17) & 7u, ib2 = (mw >> 20) & 3u;
    uint32_t pos = m + 1u;
    const uint32_t part = block_bits(lo, hi, pos, pb); pos += pb;
    const uint32_t rot = block_bits(lo, hi, pos, rb); pos += rb;
    const uint32_t isel = block_bits(lo, hi, pos, isb); pos += isb;
    // the texel's subset and the block's anchors (255: none)
    const uint32_t subset = subsets == 1u ? 0u : (subsets == 2u ? ((uint32_t)t->part2[part] >> n) & 1u : (t->part3[part] >> (2u * n)) & 3u);
    const uint32_t a1 = subsets == 1u ? 255u : (subsets == 2u ? t->anchor2[part] : t->anchor3a[part]);
    const uint32_t a2 = subsets == 3u ? t->anchor3b[part] : 255u;
    // the subset's two endpoints lie side by side in every channel's run of 2 * subsets fields
    const uint32_t ne = 2u * subsets, e = 2u * subset, both = (1u << cb) - 1u;
    const uint32_t rr = block_bits(lo, hi, pos + e * cb, 2u * cb);
    const uint32_t gg = block_bits(lo, hi, pos + (ne + e) * cb, 2u * cb);
    const uint32_t bb = block_bits(lo, hi, pos + (2u * ne + e) * cb, 2u * cb);
    pos += 3u * ne * cb;
    const uint32_t aa = block_bits(lo, hi, pos + e * ab, 2u * ab);
    pos += ne * ab;
    uint32_t r0 = rr & both, r1 = rr >> cb, g0 = gg & both, g1 = gg >> cb, b0 = bb & both, b1 = bb >> cb, al0 = aa & ((1u << ab) - 1u), al1 = aa >> ab;
    uint32_t cbits = cb, abits = ab;
    if (epb != 0u || spb != 0u) { // a p-bit goes below the stored bits
        const uint32_t p0 = block_bits(lo, hi, pos + (epb != 0u ? e : subset), 1u), p1 = epb != 0u ? block_bits(lo, hi, pos + e + 1u, 1u) : p0;
        r0 = (r0 << 1) | p0; g0 = (g0 << 1) | p0; b0 = (b0 << 1) | p0;
        r1 = (r1 << 1) | p1; g1 = (g1 << 1) | p1; b1 = (b1 << 1) | p1;
        cbits += 1u;
        if (epb != 0u && ab != 0u) { al0 = (al0 << 1) | p0; al1 = (al1 << 1) | p1; abits += 1u; }
        pos += epb != 0u ? ne : subsets;
    }
    r0 = expand_endpoint(r0, cbits); r1 = expand_endpoint(r1, cbits);
    g0 = expand_endpoint(g0, cbits); g1 = expand_endpoint(g1, cbits);
    b0 = expand_endpoint(b0, cbits); b1 = expand_endpoint(b1, cbits);
    if (ab != 0u) { al0 = expand_endpoint(al0, abits); al1 = expand_endpoint(al1, abits); }
    else al0 = al1 = 255u;
    // an anchor has one index bit fewer; the fields in front of texel n are shorter by the anchors among them
    const uint32_t anchor = (n == 0u || n == a1 || n == a2) ? 1u : 0u;
    const uint32_t before = (n > 0u ? 1u : 0u) + (n > a1 ? 1u : 0u) + (n > a2 ? 1u : 0u); // (255 is never below n)
    const uint32_t first = block_bits(lo, hi, pos + n * ib - before, ib - anchor);
    pos += 16u * ib - subsets;
    const uint32_t w1 = t->weights[(ib == 2u ? 0u : (ib == 3u ? 4u : 12u)) + first];
    uint32_t w2 = w1;
    if (ib2 != 0u) {
        const uint32_t second = block_bits(lo, hi, pos + n * ib2 - (n > 0u ? 1u : 0u), ib2 - (n == 0u ? 1u : 0u));
        w2 = t->weights[(ib2 == 2u ? 0u : 4u) + second];
    }
    const uint32_t wc = isel != 0u ? w2 : w1, wa = isel != 0u ? w1 : w2;
    uint32_t r = interpolate(r0, r1, wc), g = interpolate(g0, g1, wc), b = interpolate(b0, b1, wc), a = interpolate(al0, al1, wa);
    if (rot == 1u) { const uint32_t s = a; a = r; r = s; }
    else if (rot == 2u) { const uint32_t s = a; a = g; g = s; }
    else if (rot == 3u) { const uint32_t s = a; a = b; b = s; }
    return r | (g << 8) | (b << 16) | (a << 24);
}

// ---- BC2: 16 four-bit alphas, texel n at bits 4n, A = a * 17, in front of a colour block in the forced four-colour mode; BC4: one alpha-style block
UR_BC_FN uint32_t bc2_word(uint64_t lo, uint64_t hi, uint32_t n) { return (colour_word(hi, n, true) & 0x00FFFFFFu) | ((((uint32_t)(lo >> (4u * n)) & 15u) * 17u) << 24); }
UR_BC_FN uint32_t bc4_word(uint64_t lo, uint32_t n) { return alpha_code(lo, n) | 0xFF000000u; }

// ---- the code word of texel n over the ten source formats; `hi` is not looked at for the 8-byte formats, `t` only for BC7
UR_BC_FN uint32_t source_word(uint32_t format, uint64_t lo, uint64_t hi, uint32_t n, const WideTables* t)
{
    if (is_bc(format)) return texel_word(format, lo, hi, n);
    if (is_bc2(format)) return bc2_word(lo, hi, n);
    if (format == kBC4) return bc4_word(lo, n);
    return bc7_word(lo, hi, n, t);
}

} // namespace ur_bc
