// The host face of csrc/bc_decode.h (include/ur_host.h): the size of a BC chain and the decode of one level to RGBA8 code words, over
// the functions the sampler's kernels run (csrc/texture_sample.h). Plain C++: any compiler builds it, and the CPU tests call it.
// Behind them the same two over the ten source formats of the texture transcode (csrc/bc_wide_decode.h).

#include "../../include/ur_host.h"
#include "bc_wide_decode.h"

extern "C" {

uint64_t ur_host_bc_chain_bytes(uint32_t format, uint32_t width, uint32_t height, uint32_t mips)
{
    if (!ur_bc::is_bc(format) || width == 0u || height == 0u || width > 65535u || height > 65535u || mips == 0u || mips > 255u) return 0u;
    return (uint64_t)ur_bc::chain_bytes(format, width, height, mips);
}

int ur_host_bc_decode_level(uint32_t format, const void* blocks, uint32_t level_width, uint32_t level_height, uint8_t* rgba8_out)
{
    if (!ur_bc::is_bc(format)) return UR_EINVAL;
    return ur_host_texture_decode_level(format, blocks, level_width, level_height, rgba8_out); // (source_word is texel_word for these five)
}

uint64_t ur_host_texture_chain_bytes(uint32_t format, uint32_t width, uint32_t height, uint32_t mips)
{
    if (!ur_bc::is_source(format) || width == 0u || height == 0u || width > 65535u || height > 65535u || mips == 0u || mips > 255u) return 0u;
    return (uint64_t)ur_bc::source_chain_bytes(format, width, height, mips);
}

int ur_host_texture_decode_level(uint32_t format, const void* blocks, uint32_t level_width, uint32_t level_height, uint8_t* rgba8_out)
{
    if (!blocks || !rgba8_out || !ur_bc::is_source(format) || level_width == 0u || level_height == 0u) return UR_EINVAL;
    const uint8_t* bytes = static_cast<const uint8_t*>(blocks);
    const uint32_t across = ur_bc::blocks_across(level_width), size = ur_bc::source_block_bytes(format);
    for (uint32_t y = 0u; y < level_height; ++y) {
        for (uint32_t x = 0u; x < level_width; ++x) {
            const uint8_t* block = bytes + ur_bc::block_of(x, y, across) * size;
            uint64_t half[2] = {0u, 0u}; // little-endian halves, assembled from bytes: the host's own byte order does not matter
            for (uint32_t k = 0u; k < size; ++k) half[k >> 3] |= (uint64_t)block[k] << (8u * (k & 7u));
            const uint32_t word = ur_bc::source_word(format, half[0], half[1], ur_bc::index_in_block(x, y), &ur_bc::kWideTables);
            uint8_t* out = rgba8_out + 4u * ((size_t)y * level_width + x);
            out[0] = (uint8_t)word; out[1] = (uint8_t)(word >> 8); out[2] = (uint8_t)(word >> 16); out[3] = (uint8_t)(word >> 24);
        }
    }
    return UR_OK;
}

} // extern "C"
