// The block-compressed texel formats of the material sampler (DESIGN.md section 3.13 is the rule, tests/bcn_ref.py the restatement): the
// layout of a chain of BC1 / BC3 / BC5 levels and "the RGBA8 code word of texel n of this block", as plain inline functions with no HIP
// intrinsic. csrc/texture_sample.h (device) and csrc/bc_host.cpp (host, any C++ compiler) include this very file, so the CPU tests run
// the code the kernels run. A block is passed as its little-endian 64-bit halves: `lo` = bytes 0-7, `hi` = bytes 8-15.
// No array is indexed by a run-time value (it would become scratch): palette entries come from weights and selects, and the divisions
// by 3, 5 and 7 are multiply-and-shift, exact over the sums that occur here (tests/test_bcn_ref.py goes through every one of them).
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define UR_BC_FN __host__ __device__ inline
#else
#define UR_BC_FN inline
#endif

namespace ur_bc {

constexpr uint32_t kBC1 = 71u, kBC1Srgb = 72u, kBC3 = 77u, kBC3Srgb = 78u, kBC5 = 83u; // DXGI_FORMAT_BC*_UNORM[_SRGB]

UR_BC_FN bool is_bc1(uint32_t format) { return format == kBC1 || format == kBC1Srgb; }
UR_BC_FN bool is_bc3(uint32_t format) { return format == kBC3 || format == kBC3Srgb; }
UR_BC_FN bool is_bc(uint32_t format) { return is_bc1(format) || is_bc3(format) || format == kBC5; }
UR_BC_FN bool is_srgb(uint32_t format) { return format == 29u || format == kBC1Srgb || format == kBC3Srgb; }
// bytes of a block of a BC format (8 or 16); 0 for any other format
UR_BC_FN uint32_t block_bytes(uint32_t format) { return is_bc1(format) ? 8u : (is_bc3(format) || format == kBC5 ? 16u : 0u); }

// ---- layout: level k of a width x height chain; a dimension is at most 65535, so every level from 16 on is one texel, one block
UR_BC_FN uint32_t level_size(uint32_t size, uint32_t k) { const uint32_t s = size >> (k < 16u ? k : 16u); return s > 1u ? s : 1u; }
UR_BC_FN uint32_t blocks_across(uint32_t texels) { return (texels + 3u) >> 2; }
UR_BC_FN size_t level_blocks(uint32_t width, uint32_t height, uint32_t k) { return (size_t)blocks_across(level_size(width, k)) * blocks_across(level_size(height, k)); }
// blocks in front of level d = blocks of a chain of d levels
UR_BC_FN size_t chain_blocks(uint32_t width, uint32_t height, uint32_t d)
{
    size_t blocks = 0u;
    for (uint32_t k = 0u; k < d; ++k) blocks += level_blocks(width, height, k);
    return blocks;
}
UR_BC_FN size_t level_offset_bytes(uint32_t format, uint32_t width, uint32_t height, uint32_t d) { return chain_blocks(width, height, d) * block_bytes(format); }
UR_BC_FN size_t chain_bytes(uint32_t format, uint32_t width, uint32_t height, uint32_t mips) { return chain_blocks(width, height, mips) * block_bytes(format); }
// texel (x, y) of a level `across` blocks wide: its block, and its index inside the block
UR_BC_FN size_t block_of(uint32_t x, uint32_t y, uint32_t across) { return (size_t)(y >> 2) * across + (x >> 2); }
UR_BC_FN uint32_t index_in_block(uint32_t x, uint32_t y) { return 4u * (y & 3u) + (x & 3u); }

// ---- truncating divisions of the sums below: x <= 3 * 255, 5 * 255, 7 * 255
UR_BC_FN uint32_t div3(uint32_t x) { return (x * 43691u) >> 17; }
UR_BC_FN uint32_t div5(uint32_t x) { return (x * 52429u) >> 18; }
UR_BC_FN uint32_t div7(uint32_t x) { return (x * 9363u) >> 16; }

// ---- a colour block (BC1's 8 bytes, BC3's bytes 8-15): c0, c1 little-endian u16, then 16 2-bit indices, texel n at bits 2n.
// The RGBA8 code word of texel n, R in the low byte; `four` forces the four-colour mode (BC3). Alpha is 255, or 0 for index 3 of the
// three-colour mode (c0 <= c1).
UR_BC_FN uint32_t colour_word(uint64_t block, uint32_t n, bool four)
{
    const uint32_t ends = (uint32_t)block, c0 = ends & 0xFFFFu, c1 = ends >> 16;
    const uint32_t index = ((uint32_t)(block >> 32) >> (2u * n)) & 3u;
    four = four || c0 > c1;
    // the weight of P0 over a denominator of 3 (four colours: 3, 0, 2, 1) or 2 (three colours: 2, 0, 1, and index 3 is transparent black)
    const uint32_t den = four ? 3u : 2u;
    const uint32_t w0 = index == 0u ? den : (index == 1u ? 0u : (four ? 4u - index : 1u)), w1 = den - w0;
    const uint32_t r0 = c0 >> 11, g0 = (c0 >> 5) & 63u, b0 = c0 & 31u, r1 = c1 >> 11, g1 = (c1 >> 5) & 63u, b1 = c1 & 31u;
    const uint32_t R0 = (r0 << 3) | (r0 >> 2), G0 = (g0 << 2) | (g0 >> 4), B0 = (b0 << 3) | (b0 >> 2);
    const uint32_t R1 = (r1 << 3) | (r1 >> 2), G1 = (g1 << 2) | (g1 >> 4), B1 = (b1 << 3) | (b1 >> 2);
    const uint32_t sr = w0 * R0 + w1 * R1, sg = w0 * G0 + w1 * G1, sb = w0 * B0 + w1 * B1;
    const uint32_t r = four ? div3(sr) : sr >> 1, g = four ? div3(sg) : sg >> 1, b = four ? div3(sb) : sb >> 1;
    const uint32_t word = r | (g << 8) | (b << 16) | 0xFF000000u;
    return !four && index == 3u ? 0u : word;
}

// ---- an alpha-style block (BC3's bytes 0-7, either half of BC5): a0, a1, then 16 3-bit indices, texel n at bits 3n of the 48-bit word
UR_BC_FN uint32_t alpha_code(uint64_t block, uint32_t n)
{
    const uint32_t a0 = (uint32_t)block & 255u, a1 = ((uint32_t)block >> 8) & 255u;
    const uint32_t k = (uint32_t)(block >> (16u + 3u * n)) & 7u;
    const bool eight = a0 > a1;
    // the weight of a0 over a denominator of 7 (eight entries) or 5 (six entries, then 0 and 255)
    const uint32_t den = eight ? 7u : 5u;
    const uint32_t w0 = k == 0u ? den : (k == 1u ? 0u : den + 1u - k), w1 = den - w0; // (k = 6, 7 of the six-entry mode are replaced below)
    const uint32_t sum = w0 * a0 + w1 * a1;
    const uint32_t code = eight ? div7(sum) : div5(sum);
    return !eight && k >= 6u ? (k == 6u ? 0u : 255u) : code;
}

// ---- the code word of texel n per format; `lo` = bytes 0-7 of the block, `hi` = bytes 8-15 (not looked at for BC1)
UR_BC_FN uint32_t bc1_word(uint64_t lo, uint32_t n) { return colour_word(lo, n, false); }
UR_BC_FN uint32_t bc3_word(uint64_t lo, uint64_t hi, uint32_t n) { return (colour_word(hi, n, true) & 0x00FFFFFFu) | (alpha_code(lo, n) << 24); }
UR_BC_FN uint32_t bc5_word(uint64_t lo, uint64_t hi, uint32_t n) { return alpha_code(lo, n) | (alpha_code(hi, n) << 8) | 0xFF000000u; }
UR_BC_FN uint32_t texel_word(uint32_t format, uint64_t lo, uint64_t hi, uint32_t n)
{
    return is_bc1(format) ? bc1_word(lo, n) : (is_bc3(format) ? bc3_word(lo, hi, n) : bc5_word(lo, hi, n));
}

} // namespace ur_bc
