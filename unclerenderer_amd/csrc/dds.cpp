// DDS container parse + BC6H (UF16/SF16) block decode to RGBA16F, and RG16 pass-through — the on-disk formats of the
// lighting pass's IBL inputs: Assets/Textures/output_pmrem.dds (DX10 header, DXGI_FORMAT_BC6H_SF16,
// cube, 256^2, 9 mips) and Assets/Textures/PreintegratedGF.dds (legacy header, 32 bpp masks 0xffff/0xffff0000 =
// R16G16_UNORM, 128x32). The reference hands the compressed blocks to D3D12 and the texture unit decodes them
// (Source/Render/TextureLoader.cpp:178-315 walks the file slice-major, mips inner; DeferredRenderer.cpp:306-330 loads
// the two files); CDNA has no block-compression hardware, so the chain is decoded ONCE at setup - here on the host, staged
// with ur_stage_env_cube(), or on the device by ur_env_cube_build() (include/ur_env_cube.h), which runs the same decoder,
// csrc/bc6h_decode.h. Written from the published BC6H format description (Microsoft "BC6H Format", Khronos Data
// Format Specification §BPTC); PARITY UNPINNED: no decoder or decoded image ships with the reference.

#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/ur_assets.h"
#include "bc6h_decode.h"

namespace {

constexpr uint32_t kMagic = 0x20534444u; // "DDS "
constexpr uint32_t kFourCC_DX10 = 0x30315844u;
constexpr uint32_t DDPF_FOURCC = 0x4u, DDPF_RGB = 0x40u;
constexpr uint32_t DDSCAPS2_CUBEMAP = 0x200u;
constexpr uint32_t DXGI_R16G16B16A16_FLOAT = 10, DXGI_R16G16_UNORM = 35, DXGI_BC6H_UF16 = 95, DXGI_BC6H_SF16 = 96;

uint32_t rd32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

// ---- BC6H: csrc/bc6h_decode.h, the file the device build of the environment cube decodes with (csrc/env_cube_build.hip) -----------------
// Decode one 16-byte block into 16 texels (row-major 4x4), alpha = 1.0. Returns false on a reserved mode.
// endpoints_out (nullable): the unquantized endpoints r[4], g[4], b[4] (subset 0: [0],[1]; subset 1: [2],[3]); mode_out
// (nullable): the mode number 1..14 (0 = reserved).
bool decode_bc6h_block(const uint8_t* block, bool is_signed, ur_half4 out[16], int32_t* endpoints_out = nullptr, int* mode_out = nullptr)
{
    uint64_t lo, hi;
    std::memcpy(&lo, block, 8);
    std::memcpy(&hi, block + 8, 8);
    ur_bc6h::Header h;
    const bool ok = ur_bc6h::decode_header(lo, hi, is_signed, h);
    if (mode_out) *mode_out = ok ? ur_bc6h::kTables.mode_number[h.mode] : 0;
    if (endpoints_out) {
        const int32_t e[12] = {h.r0, h.r1, h.r2, h.r3, h.g0, h.g1, h.g2, h.g3, h.b0, h.b1, h.b2, h.b3};
        std::memcpy(endpoints_out, e, sizeof e);
    }
    for (uint32_t i = 0; i < 16; ++i) {
        const uint64_t t = ok ? ur_bc6h::texel(h, lo, hi, i, is_signed, &ur_bc6h::kTables) : ur_bc6h::kReservedTexel;
        out[i] = {(uint16_t)t, (uint16_t)(t >> 16), (uint16_t)(t >> 32), (uint16_t)(t >> 48)};
    }
    return ok;
}

uint32_t mip_dim(uint32_t base, uint32_t m) { return (base >> m) > 1u ? (base >> m) : 1u; }

} // namespace

extern "C" {

int ur_dds_parse(const void* file, size_t size, ur_dds_info* out)
{
    if (!file || !out || size < 128) return UR_ASSET_EINVAL;
    const uint8_t* p = static_cast<const uint8_t*>(file);
    if (rd32(p) != kMagic || rd32(p + 4) != 124) return UR_ASSET_EFORMAT;
    ur_dds_info d{};
    d.height = rd32(p + 12);
    d.width = rd32(p + 16);
    d.mip_count = rd32(p + 28) ? rd32(p + 28) : 1u;
    const uint32_t pf_flags = rd32(p + 80), fourcc = rd32(p + 84), rgb_bits = rd32(p + 88);
    const uint32_t rmask = rd32(p + 92), gmask = rd32(p + 96), bmask = rd32(p + 100), amask = rd32(p + 104);
    const uint32_t caps2 = rd32(p + 112);
    d.header_size = 128;
    d.slices = 1;
    d.is_cube = (caps2 & DDSCAPS2_CUBEMAP) ? 1u : 0u;
    if ((pf_flags & DDPF_FOURCC) && fourcc == kFourCC_DX10) {
        if (size < 148) return UR_ASSET_EFORMAT;
        d.header_size = 148;
        d.dxgi_format = rd32(p + 128);
        const uint32_t misc = rd32(p + 136), array_size = rd32(p + 140);
        if (misc & 0x4u) d.is_cube = 1u; // D3D10_RESOURCE_MISC_TEXTURECUBE
        d.slices = array_size ? array_size : 1u;
    } else if ((pf_flags & DDPF_RGB) && rgb_bits == 32 && rmask == 0x0000FFFFu && gmask == 0xFFFF0000u && bmask == 0 && amask == 0) {
        d.dxgi_format = DXGI_R16G16_UNORM;
    } else if ((pf_flags & DDPF_FOURCC) && fourcc == 113u) {
        d.dxgi_format = DXGI_R16G16B16A16_FLOAT; // D3DFMT_A16B16G16R16F
    } else {
        return UR_ASSET_EUNSUPPORTED;
    }
    if (d.is_cube) d.slices *= 6u;
    switch (d.dxgi_format) {
    case DXGI_BC6H_UF16:
    case DXGI_BC6H_SF16: d.block_dim = 4; d.bytes_per_block = 16; break;
    case DXGI_R16G16B16A16_FLOAT: d.block_dim = 1; d.bytes_per_block = 8; break;
    case DXGI_R16G16_UNORM: d.block_dim = 1; d.bytes_per_block = 4; break;
    default: return UR_ASSET_EUNSUPPORTED;
    }
    if (d.width == 0 || d.height == 0 || d.mip_count > 16) return UR_ASSET_EFORMAT;
    // the file must hold every subresource: slices outer, mips inner (TextureLoader.cpp:276-315)
    size_t need = d.header_size;
    for (uint32_t m = 0; m < d.mip_count; ++m) {
        const size_t bw = (mip_dim(d.width, m) + d.block_dim - 1) / d.block_dim, bh = (mip_dim(d.height, m) + d.block_dim - 1) / d.block_dim;
        need += (size_t)d.slices * bw * bh * d.bytes_per_block;
    }
    if (need > size) return UR_ASSET_EFORMAT;
    *out = d;
    return UR_ASSET_OK;
}

// A material texture: what the sampler of the raster passes takes (include/ur_raster.h), in the container forms the reference's loader
// meets (Source/Render/TextureLoader.cpp:42-63, 178-315). The payload behind the header is the device buffer as it lies.
// `source`: the formats that only ur_texture_transcode takes (BC2, BC4_UNORM, BC7) pass too.
static int parse_texture2d(const void* file, size_t size, ur_dds_info* out, bool source)
{
    if (!file || !out || size < 128) return UR_ASSET_EINVAL;
    const uint8_t* p = static_cast<const uint8_t*>(file);
    if (rd32(p) != kMagic || rd32(p + 4) != 124) return UR_ASSET_EFORMAT;
    ur_dds_info d{};
    d.height = rd32(p + 12);
    d.width = rd32(p + 16);
    d.mip_count = rd32(p + 28) ? rd32(p + 28) : 1u;
    const uint32_t pf_flags = rd32(p + 80), fourcc = rd32(p + 84), caps2 = rd32(p + 112);
    d.header_size = 128;
    d.slices = 1;
    if (caps2 & (DDSCAPS2_CUBEMAP | 0x200000u)) return UR_ASSET_EUNSUPPORTED; // a cube or a volume
    if (!(pf_flags & DDPF_FOURCC)) return UR_ASSET_EUNSUPPORTED;
    if (fourcc == kFourCC_DX10) {
        if (size < 148) return UR_ASSET_EFORMAT;
        d.header_size = 148;
        d.dxgi_format = rd32(p + 128);
        const uint32_t dimension = rd32(p + 132), misc = rd32(p + 136), array_size = rd32(p + 140);
        if (dimension != 3u || (misc & 0x4u) || array_size > 1u) return UR_ASSET_EUNSUPPORTED; // not TEXTURE2D, a cube, an array
    } else if (fourcc == 0x31545844u) d.dxgi_format = 71u; // "DXT1"
    else if (fourcc == 0x35545844u) d.dxgi_format = 77u;   // "DXT5"
    else if (fourcc == 0x32495441u || fourcc == 0x55354342u) d.dxgi_format = 83u; // "ATI2", "BC5U"
    else if (source && fourcc == 0x33545844u) d.dxgi_format = 74u;                // "DXT3"
    else if (source && (fourcc == 0x31495441u || fourcc == 0x55344342u)) d.dxgi_format = 80u; // "ATI1", "BC4U"
    else return UR_ASSET_EUNSUPPORTED;
    switch (d.dxgi_format) {
    case 28u: case 29u: d.block_dim = 1; d.bytes_per_block = 4; break;
    case 71u: case 72u: d.block_dim = 4; d.bytes_per_block = 8; break;
    case 77u: case 78u: case 83u: d.block_dim = 4; d.bytes_per_block = 16; break;
    case 80u: if (!source) return UR_ASSET_EUNSUPPORTED; d.block_dim = 4; d.bytes_per_block = 8; break;
    case 74u: case 75u: case 98u: case 99u: if (!source) return UR_ASSET_EUNSUPPORTED; d.block_dim = 4; d.bytes_per_block = 16; break;
    default: return UR_ASSET_EUNSUPPORTED;
    }
    if (d.width == 0 || d.height == 0 || d.width > 65535u || d.height > 65535u || d.mip_count > 255u) return UR_ASSET_EFORMAT;
    size_t need = d.header_size;
    for (uint32_t m = 0; m < d.mip_count; ++m) {
        const size_t bw = (mip_dim(d.width, m < 16u ? m : 16u) + d.block_dim - 1) / d.block_dim, bh = (mip_dim(d.height, m < 16u ? m : 16u) + d.block_dim - 1) / d.block_dim;
        need += bw * bh * d.bytes_per_block;
    }
    if (need > size) return UR_ASSET_EFORMAT;
    *out = d;
    return UR_ASSET_OK;
}

int ur_dds_parse_texture2d(const void* file, size_t size, ur_dds_info* out) { return parse_texture2d(file, size, out, false); }
int ur_dds_parse_texture2d_source(const void* file, size_t size, ur_dds_info* out) { return parse_texture2d(file, size, out, true); }

size_t ur_dds_texel_count(const ur_dds_info* d)
{
    if (!d) return 0;
    size_t n = 0;
    for (uint32_t m = 0; m < d->mip_count; ++m) n += (size_t)mip_dim(d->width, m) * mip_dim(d->height, m);
    return n * d->slices;
}

int ur_dds_decode_rgba16f(const void* file, size_t size, const ur_dds_info* d, ur_half4* out, uint32_t* reserved_blocks)
{
    if (!file || !d || !out || size < d->header_size) return UR_ASSET_EINVAL;
    const bool bc6 = d->dxgi_format == DXGI_BC6H_UF16 || d->dxgi_format == DXGI_BC6H_SF16;
    if (!bc6 && d->dxgi_format != DXGI_R16G16B16A16_FLOAT) return UR_ASSET_EUNSUPPORTED;
    const bool is_signed = d->dxgi_format == DXGI_BC6H_SF16;
    const uint8_t* src = static_cast<const uint8_t*>(file) + d->header_size;
    uint32_t bad = 0;
    for (uint32_t s = 0; s < d->slices; ++s)
        for (uint32_t m = 0; m < d->mip_count; ++m) {
            const uint32_t w = mip_dim(d->width, m), h = mip_dim(d->height, m);
            if (!bc6) {
                std::memcpy(out, src, (size_t)w * h * 8);
                src += (size_t)w * h * 8;
            } else {
                const uint32_t bw = (w + 3) / 4, bh = (h + 3) / 4;
                for (uint32_t by = 0; by < bh; ++by)
                    for (uint32_t bx = 0; bx < bw; ++bx) {
                        ur_half4 texels[16];
                        if (!decode_bc6h_block(src, is_signed, texels)) ++bad;
                        src += 16;
                        for (uint32_t ty = 0; ty < 4; ++ty)
                            for (uint32_t tx = 0; tx < 4; ++tx) {
                                const uint32_t x = bx * 4 + tx, y = by * 4 + ty;
                                if (x < w && y < h) out[(size_t)y * w + x] = texels[ty * 4 + tx];
                            }
                    }
            }
            out += (size_t)w * h;
        }
    if (reserved_blocks) *reserved_blocks = bad;
    return UR_ASSET_OK;
}

int ur_dds_copy_rg16(const void* file, size_t size, const ur_dds_info* d, uint16_t* out)
{
    if (!file || !d || !out) return UR_ASSET_EINVAL;
    if (d->dxgi_format != DXGI_R16G16_UNORM) return UR_ASSET_EUNSUPPORTED;
    const size_t bytes = ur_dds_texel_count(d) * 4;
    if (d->header_size + bytes > size) return UR_ASSET_EFORMAT;
    std::memcpy(out, static_cast<const uint8_t*>(file) + d->header_size, bytes);
    return UR_ASSET_OK;
}

int ur_bc6h_decode_block(const uint8_t block[16], int is_signed, ur_half4 out[16]) { return decode_bc6h_block(block, is_signed != 0, out) ? 1 : 0; }

int ur_bc6h_block_endpoints(const uint8_t block[16], int is_signed, int32_t endpoints[12])
{
    ur_half4 texels[16];
    int mode = 0;
    decode_bc6h_block(block, is_signed != 0, texels, endpoints, &mode);
    return mode;
}

} // extern "C"
