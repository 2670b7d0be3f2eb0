/*
 * ur_assets.h — setup-time staging of the lighting pass's IBL inputs from their on-disk format:
 * DDS container parse (DX10 and legacy headers), BC6H_UF16 / BC6H_SF16 block decode to RGBA16F, R16G16_UNORM copy.
 * Host-only, no GPU. Replaces what the reference gets from D3D12 + ddspp (Source/Render/TextureLoader.cpp:178-315;
 * loads at DeferredRenderer.cpp:306-330): the decoded chain is in the same order the loader walks the file
 * (slice-major, mips inner) — exactly what ur_stage_env_cube() takes.
 */
#ifndef UR_ASSETS_H
#define UR_ASSETS_H

#include <stddef.h>
#include <stdint.h>

#include "ur_hotpath.h"

#ifdef __cplusplus
extern "C" {
#endif

#define UR_ASSET_OK 0
#define UR_ASSET_EINVAL (-1)
#define UR_ASSET_EFORMAT (-2)      /* not a DDS file / truncated */
#define UR_ASSET_EUNSUPPORTED (-3) /* a pixel format other than BC6H, RGBA16F, RG16 */

typedef struct ur_dds_info {
    uint32_t width, height, mip_count;
    uint32_t slices;          /* array size x 6 for cubes */
    uint32_t is_cube;
    uint32_t dxgi_format;     /* 95 BC6H_UF16, 96 BC6H_SF16, 10 R16G16B16A16_FLOAT, 35 R16G16_UNORM */
    uint32_t header_size;     /* 128, or 148 with the DX10 extension */
    uint32_t block_dim;       /* 4 for BC6H, 1 otherwise */
    uint32_t bytes_per_block; /* 16 / 8 / 4 */
} ur_dds_info;

int ur_dds_parse(const void* file, size_t size, ur_dds_info* out);
/* A material texture for the sampler of the raster passes (ur_texture2d in ur_raster.h): a 2D DDS - no cube, no array, no volume - of
 * DXGI format 28, 29 (R8G8B8A8_UNORM[_SRGB]), 71, 72 (BC1), 77, 78 (BC3) or 83 (BC5_UNORM), in a DX10 header or as the legacy FourCCs
 * "DXT1" (71), "DXT5" (77), "ATI2" and "BC5U" (83). Fills `out` (slices 1, is_cube 0; block_dim 4 and 8 or 16 bytes per block for BC,
 * 1 and 4 for RGBA8). The mip chain behind header_size is in ur_texture2d's order and pitch: the payload is the device buffer.
 * UR_ASSET_EUNSUPPORTED for any other format or shape, UR_ASSET_EFORMAT for a file that is not DDS, a dimension above 65535, more than
 * 255 mips or a payload shorter than the chain. */
int ur_dds_parse_texture2d(const void* file, size_t size, ur_dds_info* out);
/* A source of ur_texture_transcode (include/ur_raster.h): everything ur_dds_parse_texture2d accepts, plus DXGI 74, 75 (BC2), 80
 * (BC4_UNORM), 98 and 99 (BC7), in a DX10 header or as the legacy FourCCs "DXT3" (74), "ATI1" and "BC4U" (80); 8 bytes a block for BC4,
 * 16 for BC2 and BC7. The payload behind header_size is the source chain as it lies. The SNORM forms, BC6H, cubes, arrays and volumes
 * stay UR_ASSET_EUNSUPPORTED; the other refusals are ur_dds_parse_texture2d's. */
int ur_dds_parse_texture2d_source(const void* file, size_t size, ur_dds_info* out);
/* texels of the whole chain (all slices, all mips) */
size_t ur_dds_texel_count(const ur_dds_info* info);
/* BC6H / RGBA16F file -> RGBA16F texels, slice-major, mips inner, rows top-down. reserved_blocks (nullable) counts BC6H
 * blocks with a reserved mode (decoded as zero, like D3D). */
int ur_dds_decode_rgba16f(const void* file, size_t size, const ur_dds_info* info, ur_half4* out, uint32_t* reserved_blocks);
/* R16G16_UNORM file -> 2 x uint16 per texel */
int ur_dds_copy_rg16(const void* file, size_t size, const ur_dds_info* info, uint16_t* out);
/* one BC6H block -> 16 texels (row-major 4x4); returns 0 for a reserved mode */
int ur_bc6h_decode_block(const uint8_t block[16], int is_signed, ur_half4 out[16]);
/* the block's mode number (1..14, 0 = reserved) and its unquantized endpoints r[4], g[4], b[4] (subset 0: [0],[1]; subset 1:
 * [2],[3]; one-region modes leave [2],[3] zero) — what the decoder interpolates between; for tests and asset diagnostics */
int ur_bc6h_block_endpoints(const uint8_t block[16], int is_signed, int32_t endpoints[12]);

/* A Radiance .hdr panorama (csrc/hdr.cpp): the file's texels as they lie, four bytes R G B E each - what
 * ur_env_panorama (include/ur_env_panorama.h) takes on the device. The rule is the one stb_image's HDR loader reads by. */
#define UR_HDR_MAX_WIDTH 16384u
#define UR_HDR_MAX_HEIGHT 8192u

typedef struct ur_hdr_info {
    uint32_t width, height;
    uint32_t payload_offset; /* where the first scanline starts in the file */
    uint32_t rle;            /* 1: scanlines are run-length coded (new-style RLE); 0: the payload is flat, 4 * width * height bytes */
} ur_hdr_info;

/* The header: a first line "#?RADIANCE" or "#?RGBE", header lines up to the empty line, "FORMAT=32-bit_rle_rgbe" among them, then the
 * resolution line "-Y H +X W" with 1 <= W <= UR_HDR_MAX_WIDTH and 1 <= H <= UR_HDR_MAX_HEIGHT. The payload is run-length coded when
 * 8 <= W < 32768 and it starts 02 02 hi lo with hi < 128, flat otherwise (the first scanline decides for the file).
 * UR_EUNSUPPORTED for a resolution line of any other orientation; UR_EINVAL for a null argument, a file that is not Radiance, a header
 * that ends early, a missing FORMAT line or a size out of range. ur_hdr_last_error has the text. */
int ur_hdr_parse(const void* file, size_t size, ur_hdr_info* out);
/* Writes 4 * width * height bytes, R G B E per texel, top row first. A flat payload is copied. A run-length coded one is expanded
 * scanline by scanline: the marker 02 02 hi lo with (hi << 8 | lo) == width, then for each of the four channel planes count bytes - above
 * 128 a run of count - 128 copies of the next byte, otherwise that many literal bytes. UR_EINVAL (ur_hdr_last_error has the text) for a
 * null argument, an info that is not ur_hdr_parse's of this file, a count of 0, a run or literals past the width, a later scanline
 * without the marker or with another length, and a truncated file; rgbe_out is then unspecified but never written outside its bytes. */
int ur_hdr_unpack(const void* file, size_t size, const ur_hdr_info* info, uint8_t* rgbe_out);
/* The text of the calling thread's last refusal by ur_hdr_parse or ur_hdr_unpack ("" before the first). */
const char* ur_hdr_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* UR_ASSETS_H */
