/*
 * ur_brdf_lut.h - the BRDF LUT: the split-sum table of the specular image-based lighting (the scale and bias of F0 over NoV and
 * roughness), computed on the device in one asynchronous call with nothing read back. The result - width x height
 * texels of 2 x UNORM16, row-major - is exactly what ur_lighting_tables.brdf_lut_rg16 takes; at 128 x 32 it is what the streaming
 * lighting kernel requires and what the shipped PreintegratedGF.dds holds by the same rule: column x is NoV = (x + 0.5) / width, row y
 * is roughness = (y + 0.5) / height with alpha = roughness^2, the GGX distribution is importance-sampled at sample_count Hammersley
 * points, the visibility is the approximated joint Smith term 0.5 / (NoL (NoV (1 - alpha) + alpha) + NoV (NoL (1 - alpha) + alpha)).
 * The same rule in plain serial C++ is ur_host_brdf_lut (include/ur_host.h).
 */
#ifndef UR_BRDF_LUT_H
#define UR_BRDF_LUT_H

#include <stddef.h>
#include <stdint.h>

#include "ur_hotpath.h"

#ifdef __cplusplus
extern "C" {
#endif

#define UR_BRDF_LUT_MAX_WIDTH 1024u
#define UR_BRDF_LUT_MAX_HEIGHT 256u
#define UR_BRDF_LUT_MIN_SAMPLES 16u
#define UR_BRDF_LUT_MAX_SAMPLES 4096u
/* ur_brdf_lut puts at most this many operations on the context's stream, whatever the sizes: one launch. */
#define UR_BRDF_LUT_MAX_STREAM_OPS 1u

/* Bytes of the sample table of a LUT of `height` rows and sample_count samples a texel: 16 * height * sample_count (sixteen bytes
 * {hx, hy, hz, 0} a row and sample; ur_host_brdf_lut_table of include/ur_host.h fills it). 0 for a height outside
 * 1..UR_BRDF_LUT_MAX_HEIGHT or a sample_count that is no power of two in UR_BRDF_LUT_MIN_SAMPLES..UR_BRDF_LUT_MAX_SAMPLES. */
size_t ur_brdf_lut_table_bytes(uint32_t height, uint32_t sample_count);

/* Builds the table on the context's stream: asynchronous, no host allocation, no copy, no scratch, the host reads no device memory and
 * does not synchronise; at most UR_BRDF_LUT_MAX_STREAM_OPS stream operations. Device memory: table_device (at least
 * ur_brdf_lut_table_bytes(height, sample_count) bytes, only those are read), dst_device (dst_bytes = 4 * width * height: every byte is
 * written, so what it holds on entry does not matter); both 16-byte aligned.
 * UR_EINVAL (ur_last_error has the text), decided from the arguments alone, nothing launched: a null context or pointer; a width outside
 * 1..UR_BRDF_LUT_MAX_WIDTH or a height outside 1..UR_BRDF_LUT_MAX_HEIGHT; a sample_count that is no power of two in 16..4096; a table
 * shorter than ur_brdf_lut_table_bytes; dst_bytes that is not the table's; a pointer that is not 16-byte aligned; table and destination
 * overlapping. */
int ur_brdf_lut(ur_ctx* ctx, uint32_t width, uint32_t height, uint32_t sample_count, const void* table_device, size_t table_bytes, void* dst_device,
                size_t dst_bytes);

#ifdef __cplusplus
}
#endif
#endif /* UR_BRDF_LUT_H */
