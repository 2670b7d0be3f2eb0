// BC6H (UF16 / SF16), the block format of the environment cube (DESIGN.md sections 3.19 and 7): the 14 modes, the two-subset partition
// rows, sign extension, the two unquantize steps, the reserved modes as zero - as plain inline functions with no HIP intrinsic.
// csrc/dds.cpp and csrc/env_cube_host.cpp (host, any C++ compiler) and csrc/env_cube_build.hip (device) include this very file, so the CPU
// tests (tests/golden/bc6h_pillow.npz among them) run the code the kernel runs. Written from the published format description
// (Microsoft "BC6H Format", Khronos Data Format Specification, BPTC).
// A block is passed as its little-endian 64-bit halves: `lo` = bytes 0-7, `hi` = bytes 8-15. It is decoded in two steps: the header -
// mode, partition, the unquantized endpoints - once, then any texel from the header and the texel's own index bits, which are found by
// position: no texel waits for the one in front of it. No array is indexed by a run-time value (it would become scratch on the device):
// every field of a mode sits at a position the compiler knows, endpoints are chosen by selects, and the tables - partition rows, anchors,
// weights, mode numbers - are one packed struct of 160 bytes passed by pointer: the host passes kTables itself, a kernel a copy in LDS.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define UR_BC6H_FN __host__ __device__ inline
#else
#define UR_BC6H_FN inline
#endif

namespace ur_bc6h {

struct Tables {
    uint16_t part2[32];      // two subsets: texel n's subset at bit n (the first 32 shapes of the BPTC set)
    uint8_t anchor2[32];     // the anchor (fix-up) texel of subset 1
    uint8_t weights3[8];     // 3-bit indices
    uint8_t weights4[16];    // 4-bit indices
    uint8_t mode_number[32]; // the five mode bits -> 1..14, 0 = reserved
    uint8_t pad[8];
};
static_assert(sizeof(Tables) == 160, "staged as 40 dwords");
constexpr Tables kTables = {
    {0xCCCC, 0x8888, 0xEEEE, 0xECC8, 0xC880, 0xFEEC, 0xFEC8, 0xEC80, 0xC800, 0xFFEC, 0xFE80, 0xE800, 0xFFE8, 0xFF00, 0xFFF0, 0xF000,
     0xF710, 0x008E, 0x7100, 0x08CE, 0x008C, 0x7310, 0x3100, 0x8CCE, 0x088C, 0x3110, 0x6666, 0x366C, 0x17E8, 0x0FF0, 0x718E, 0x399C},
    {15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 2, 8, 2, 2, 8, 8, 15, 2, 8, 2, 2, 8, 8, 2, 2},
    {0, 9, 18, 27, 37, 46, 55, 64},
    {0, 4, 9, 13, 17, 21, 26, 30, 34, 38, 43, 47, 51, 55, 60, 64},
    {1, 2, 3, 11, 0, 0, 4, 12, 0, 0, 5, 13, 0, 0, 6, 14, 0, 0, 7, 0, 0, 0, 8, 0, 0, 0, 9, 0, 0, 0, 10, 0},
    {0, 0, 0, 0, 0, 0, 0, 0}};

// Is the block whose first byte is `byte0` of a reserved mode? Modes 1 and 2 have two mode bits (00, 01), the rest five; of the five-bit
// codes that end in 11, those with bit 4 set are reserved. decode_header's switch is the rule; tests hold the two to each other.
UR_BC6H_FN bool reserved_mode(uint32_t byte0) { return (byte0 & 0x13u) == 0x13u; }

struct BitReader {
    uint64_t lo, hi;
    uint32_t pos;
    UR_BC6H_FN uint32_t bits(uint32_t n) // 1..10 bits, least significant first
    {
        const uint64_t v = pos >= 64u ? hi >> (pos - 64u) : (lo >> pos) | ((hi << 1) << (63u - pos));
        pos += n;
        return (uint32_t)v & ((1u << n) - 1u);
    }
    UR_BC6H_FN uint32_t bit() { return bits(1u); }
    UR_BC6H_FN uint32_t bits_rev(uint32_t n) // the first bit read is the MOST significant (the spec's "[10:15]" fields)
    {
        uint32_t v = 0u;
        for (uint32_t i = 0u; i < n; ++i) v = (v << 1) | bit();
        return v;
    }
};

UR_BC6H_FN int sign_extend(int v, int bits)
{
    const int m = 1 << (bits - 1);
    v &= (1 << bits) - 1;
    return (v ^ m) - m;
}

UR_BC6H_FN int unquantize(int x, int bits, bool is_signed)
{
    if (is_signed) {
        if (bits >= 16) return x;
        const bool neg = x < 0;
        if (neg) x = -x;
        int unq;
        if (x == 0) unq = 0;
        else if (x >= ((1 << (bits - 1)) - 1)) unq = 0x7FFF;
        else unq = ((x << 15) + 0x4000) >> (bits - 1);
        return neg ? -unq : unq;
    }
    if (bits >= 15) return x;
    if (x == 0) return 0;
    if (x == ((1 << bits) - 1)) return 0xFFFF;
    return ((x << 15) + 0x4000) >> (bits - 1);
}

UR_BC6H_FN uint32_t finish_unquantize(int v, bool is_signed)
{
    if (is_signed) {
        const bool neg = v < 0;
        if (neg) v = -v;
        v = (v * 31) >> 5;
        return (uint32_t)(neg ? (0x8000 | v) : v) & 0xFFFFu;
    }
    return (uint32_t)((v * 31) >> 6) & 0xFFFFu;
}

// A block's header: the five mode bits (those of modes 1 and 2 are 0 and 1), 1 or 2 regions, the partition, and the unquantized endpoints
// (subset 0: 0 and 1; subset 1: 2 and 3, zero in a one-region mode).
struct Header {
    int r0, r1, r2, r3, g0, g1, g2, g3, b0, b1, b2, b3;
    uint32_t mode, regions, partition;
};

// one channel's endpoints: sign extension, the delta transform, unquantization (endpoint 0 first: the others are deltas from it)
UR_BC6H_FN int finish_delta(int e0, int e, int wbits, int dbits, bool transformed, bool is_signed)
{
    if (transformed) {
        e = (e0 + sign_extend(e, dbits)) & ((1 << wbits) - 1);
        if (is_signed) e = sign_extend(e, wbits);
    } else if (is_signed) {
        e = sign_extend(e, wbits); // direct modes: delta width == endpoint width
    }
    return unquantize(e, wbits, is_signed);
}
struct Ends { int e0, e1, e2, e3; };
UR_BC6H_FN Ends finish_endpoints(int e0, int e1, int e2, int e3, int wbits, int dbits, bool transformed, bool two, bool is_signed)
{
    if (is_signed) e0 = sign_extend(e0, wbits);
    const int f1 = finish_delta(e0, e1, wbits, dbits, transformed, is_signed);
    const int f2 = finish_delta(e0, e2, wbits, dbits, transformed, is_signed), f3 = finish_delta(e0, e3, wbits, dbits, transformed, is_signed);
    if (!is_signed) e0 &= (1 << wbits) - 1;
    return Ends{unquantize(e0, wbits, is_signed), f1, two ? f2 : 0, two ? f3 : 0}; // (one region: endpoints 2 and 3 are zero)
}

// Returns false on a reserved mode: the header is zero, the block decodes to (0, 0, 0, 1).
UR_BC6H_FN bool decode_header(uint64_t lo, uint64_t hi, bool is_signed, Header& h)
{
    BitReader br = {lo, hi, 0u};
    int r0 = 0, r1 = 0, r2 = 0, r3 = 0, g0 = 0, g1 = 0, g2 = 0, g3 = 0, b0 = 0, b1 = 0, b2 = 0, b3 = 0;
    uint32_t partition = 0u;
    uint32_t mode = br.bits(2);
    if (mode > 1u) mode |= br.bits(3) << 2;
    int regions, transformed, wbits, dr, dg, db;
    // (br.pos is 2 behind modes 1 and 2 and 5 behind the rest: said again in every case, so that every field's position is a constant)
#define UR_BC6H_MODE(position, regions_, transformed_, wbits_, dr_, dg_, db_) \
    br.pos = position; regions = regions_; transformed = transformed_; wbits = wbits_; dr = dr_; dg = dg_; db = db_
#define RW(n) r0 |= (int)br.bits(n)
#define GW(n) g0 |= (int)br.bits(n)
#define BW(n) b0 |= (int)br.bits(n)
#define RX(n) r1 |= (int)br.bits(n)
#define GX(n) g1 |= (int)br.bits(n)
#define BX(n) b1 |= (int)br.bits(n)
#define RY(n) r2 |= (int)br.bits(n)
#define GY(n) g2 |= (int)br.bits(n)
#define BY(n) b2 |= (int)br.bits(n)
#define RZ(n) r3 |= (int)br.bits(n)
#define GZ(n) g3 |= (int)br.bits(n)
#define BZ(n) b3 |= (int)br.bits(n)
#define GYb(k) g2 |= (int)(br.bit() << (k))
#define BYb(k) b2 |= (int)(br.bit() << (k))
#define GZb(k) g3 |= (int)(br.bit() << (k))
#define BZb(k) b3 |= (int)(br.bit() << (k))
#define RWb(k) r0 |= (int)(br.bit() << (k))
#define GWb(k) g0 |= (int)(br.bit() << (k))
#define BWb(k) b0 |= (int)(br.bit() << (k))
    switch (mode) {
    case 0x00: // mode 1: 10.555
        UR_BC6H_MODE(2u, 2, 1, 10, 5, 5, 5);
        GYb(4); BYb(4); BZb(4); RW(10); GW(10); BW(10); RX(5); GZb(4); GY(4); GX(5); BZb(0); GZ(4); BX(5); BZb(1); BY(4); RY(5); BZb(2); RZ(5); BZb(3);
        partition = br.bits(5);
        break;
    case 0x01: // mode 2: 7.666
        UR_BC6H_MODE(2u, 2, 1, 7, 6, 6, 6);
        GYb(5); GZb(4); GZb(5); RW(7); BZb(0); BZb(1); BYb(4); GW(7); BYb(5); BZb(2); GYb(4); BW(7); BZb(3); BZb(5); BZb(4); RX(6); GY(4); GX(6); GZ(4); BX(6);
        BY(4); RY(6); RZ(6);
        partition = br.bits(5);
        break;
    case 0x02: // mode 3: 11.544
        UR_BC6H_MODE(5u, 2, 1, 11, 5, 4, 4);
        RW(10); GW(10); BW(10); RX(5); RWb(10); GY(4); GX(4); GWb(10); BZb(0); GZ(4); BX(4); BWb(10); BZb(1); BY(4); RY(5); BZb(2); RZ(5); BZb(3);
        partition = br.bits(5);
        break;
    case 0x06: // mode 4: 11.454
        UR_BC6H_MODE(5u, 2, 1, 11, 4, 5, 4);
        RW(10); GW(10); BW(10); RX(4); RWb(10); GZb(4); GY(4); GX(5); GWb(10); GZ(4); BX(4); BWb(10); BZb(1); BY(4); RY(4); BZb(0); BZb(2); RZ(4); GYb(4); BZb(3);
        partition = br.bits(5);
        break;
    case 0x0A: // mode 5: 11.445
        UR_BC6H_MODE(5u, 2, 1, 11, 4, 4, 5);
        RW(10); GW(10); BW(10); RX(4); RWb(10); BYb(4); GY(4); GX(4); GWb(10); BZb(0); GZ(4); BX(5); BWb(10); BY(4); RY(4); BZb(1); BZb(2); RZ(4); BZb(4); BZb(3);
        partition = br.bits(5);
        break;
    case 0x0E: // mode 6: 9.555
        UR_BC6H_MODE(5u, 2, 1, 9, 5, 5, 5);
        RW(9); BYb(4); GW(9); GYb(4); BW(9); BZb(4); RX(5); GZb(4); GY(4); GX(5); BZb(0); GZ(4); BX(5); BZb(1); BY(4); RY(5); BZb(2); RZ(5); BZb(3);
        partition = br.bits(5);
        break;
    case 0x12: // mode 7: 8.655
        UR_BC6H_MODE(5u, 2, 1, 8, 6, 5, 5);
        RW(8); GZb(4); BYb(4); GW(8); BZb(2); GYb(4); BW(8); BZb(3); BZb(4); RX(6); GY(4); GX(5); BZb(0); GZ(4); BX(5); BZb(1); BY(4); RY(6); RZ(6);
        partition = br.bits(5);
        break;
    case 0x16: // mode 8: 8.565
        UR_BC6H_MODE(5u, 2, 1, 8, 5, 6, 5);
        RW(8); BZb(0); BYb(4); GW(8); GYb(5); GYb(4); BW(8); GZb(5); BZb(4); RX(5); GZb(4); GY(4); GX(6); GZ(4); BX(5); BZb(1); BY(4); RY(5); BZb(2); RZ(5); BZb(3);
        partition = br.bits(5);
        break;
    case 0x1A: // mode 9: 8.556
        UR_BC6H_MODE(5u, 2, 1, 8, 5, 5, 6);
        RW(8); BZb(1); BYb(4); GW(8); BYb(5); GYb(4); BW(8); BZb(5); BZb(4); RX(5); GZb(4); GY(4); GX(5); BZb(0); GZ(4); BX(6); BY(4); RY(5); BZb(2); RZ(5); BZb(3);
        partition = br.bits(5);
        break;
    case 0x1E: // mode 10: 6.666, endpoints stored directly
        UR_BC6H_MODE(5u, 2, 0, 6, 6, 6, 6);
        RW(6); GZb(4); BZb(0); BZb(1); BYb(4); GW(6); GYb(5); BYb(5); BZb(2); GYb(4); BW(6); GZb(5); BZb(3); BZb(5); BZb(4); RX(6); GY(4); GX(6); GZ(4); BX(6);
        BY(4); RY(6); RZ(6);
        partition = br.bits(5);
        break;
    case 0x03: // mode 11: 10.10, one region, direct
        UR_BC6H_MODE(5u, 1, 0, 10, 10, 10, 10);
        RW(10); GW(10); BW(10); RX(10); GX(10); BX(10);
        break;
    case 0x07: // mode 12: 11.9
        UR_BC6H_MODE(5u, 1, 1, 11, 9, 9, 9);
        RW(10); GW(10); BW(10); RX(9); RWb(10); GX(9); GWb(10); BX(9); BWb(10);
        break;
    case 0x0B: // mode 13: 12.8
        UR_BC6H_MODE(5u, 1, 1, 12, 8, 8, 8);
        RW(10); GW(10); BW(10); RX(8); r0 |= (int)(br.bits_rev(2) << 10); GX(8); g0 |= (int)(br.bits_rev(2) << 10); BX(8); b0 |= (int)(br.bits_rev(2) << 10);
        break;
    case 0x0F: // mode 14: 16.4
        UR_BC6H_MODE(5u, 1, 1, 16, 4, 4, 4);
        RW(10); GW(10); BW(10); RX(4); r0 |= (int)(br.bits_rev(6) << 10); GX(4); g0 |= (int)(br.bits_rev(6) << 10); BX(4); b0 |= (int)(br.bits_rev(6) << 10);
        break;
    default: // reserved modes decode to zero (D3D behaviour)
        h.r0 = h.r1 = h.r2 = h.r3 = h.g0 = h.g1 = h.g2 = h.g3 = h.b0 = h.b1 = h.b2 = h.b3 = 0;
        h.mode = mode; h.regions = 0u; h.partition = 0u;
        return false;
    }
#undef UR_BC6H_MODE
#undef RW
#undef GW
#undef BW
#undef RX
#undef GX
#undef BX
#undef RY
#undef GY
#undef BY
#undef RZ
#undef GZ
#undef BZ
#undef GYb
#undef BYb
#undef GZb
#undef BZb
#undef RWb
#undef GWb
#undef BWb
    const Ends r = finish_endpoints(r0, r1, r2, r3, wbits, dr, transformed != 0, regions == 2, is_signed);
    const Ends g = finish_endpoints(g0, g1, g2, g3, wbits, dg, transformed != 0, regions == 2, is_signed);
    const Ends b = finish_endpoints(b0, b1, b2, b3, wbits, db, transformed != 0, regions == 2, is_signed);
    h.r0 = r.e0; h.r1 = r.e1; h.r2 = r.e2; h.r3 = r.e3;
    h.g0 = g.e0; h.g1 = g.e1; h.g2 = g.e2; h.g3 = g.e3;
    h.b0 = b.e0; h.b1 = b.e1; h.b2 = b.e2; h.b3 = b.e3;
    h.mode = mode; h.regions = (uint32_t)regions; h.partition = partition;
    return true;
}

// Texel i (row-major 4 x 4) of a block whose header decoded: R | G << 16 | B << 32 | 1.0 << 48, the bytes of a half4. The index bits lie
// behind the header, from bit 65 (one region: 4 bits a texel) or 82 (two: 3 bits), an anchor texel one bit short: texel i's start at
// first + width * i, less one for texel 0 in front of it and one for subset 1's anchor in front of it.
UR_BC6H_FN uint64_t texel(const Header& h, uint64_t lo, uint64_t hi, uint32_t i, bool is_signed, const Tables* t)
{
    const bool two = h.regions == 2u;
    const uint32_t anchor2 = two ? t->anchor2[h.partition] : 16u; // (16: no texel)
    const uint32_t subset = two ? (t->part2[h.partition] >> i) & 1u : 0u;
    const uint32_t width = two ? 3u : 4u;
    const bool anchor = i == 0u || i == anchor2;
    BitReader br = {lo, hi, (two ? 82u : 65u) + width * i - (i > 0u ? 1u : 0u) - (i > anchor2 ? 1u : 0u)};
    const uint32_t idx = br.bits(anchor ? width - 1u : width);
    const int w = two ? t->weights3[idx] : t->weights4[idx];
    const int r0 = subset ? h.r2 : h.r0, r1 = subset ? h.r3 : h.r1;
    const int g0 = subset ? h.g2 : h.g0, g1 = subset ? h.g3 : h.g1;
    const int b0 = subset ? h.b2 : h.b0, b1 = subset ? h.b3 : h.b1;
    const uint64_t hr = finish_unquantize((r0 * (64 - w) + r1 * w + 32) >> 6, is_signed);
    const uint64_t hg = finish_unquantize((g0 * (64 - w) + g1 * w + 32) >> 6, is_signed);
    const uint64_t hb = finish_unquantize((b0 * (64 - w) + b1 * w + 32) >> 6, is_signed);
    return hr | (hg << 16) | (hb << 32) | (0x3C00ull << 48);
}

constexpr uint64_t kReservedTexel = 0x3C00ull << 48; // (0, 0, 0, 1.0)

} // namespace ur_bc6h
