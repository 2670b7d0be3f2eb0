// The records of the post exchange (include/ur_hotpath.h: ur_pack_post_record, ur_pack_taa_record), laid out once: for the kernels that
// write and read them (csrc/post.hip, csrc/taa.hip), the two *_record_bytes entry points and the frame, which points launches at rows of
// a neighbour's record in place (csrc/frame/PostPasses.cpp). Plain C++. Not installed.
#pragma once

#include <cstdint>

namespace ur_records {

constexpr uint32_t kTexelBytes = 8u; // a record is a row of RGBA16F texels

// The post record of a band of a W-wide frame: two rows of W texels, then the 4 texels of each of AutoExposure's 256 taps in tap order.
constexpr uint32_t kPostFirstRow = 0u, kPostLastRow = 1u; // the band's first and last HDR row
constexpr uint32_t kPostRows = 2u;                        // the taps start behind them, at texel kPostRows * W
constexpr uint32_t kTapTexels = 1024u;
constexpr uint64_t post_texels(uint32_t w) { return (uint64_t)kPostRows * w + kTapTexels; }

// The TAA record: four rows of W texels.
constexpr uint32_t kTaaSecondRow = 0u, kTaaSecondLastRow = 1u; // the band's second and second-last current row
constexpr uint32_t kTaaHistFirstRow = 2u, kTaaHistLastRow = 3u; // first and last row of the history image the frame reads (zeros without)
constexpr uint32_t kTaaRows = 4u;
constexpr uint64_t taa_texels(uint32_t w) { return (uint64_t)kTaaRows * w; }

// where row `row` (one of the names above) of a record starts, in bytes from the record's first
constexpr uint64_t row_offset(uint32_t row, uint32_t w) { return (uint64_t)row * kTexelBytes * w; }

} // namespace ur_records
