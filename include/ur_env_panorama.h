/*
 * ur_env_panorama.h - environment from a panorama: the RGBE texels of a lat-long Radiance .hdr panorama (ur_hdr_unpack of
 * include/ur_assets.h: four bytes R G B E each, top row first) become the top level of an HDR cube - six square R16G16B16A16_FLOAT faces
 * of a power-of-two edge, face-major, alpha 1.0 - on the device, in one asynchronous call with nothing read back.
 * The result is exactly the source of ur_env_prefilter (include/ur_env_prefilter.h):
 *     .hdr file -> ur_hdr_unpack -> ur_env_panorama -> ur_env_prefilter -> ur_env_cube_build -> Lighting / Forward.
 * The panorama's centre column looks along +Z, u grows towards +X, row 0 is +Y. A texel is m * 2^(e - 136) per channel (0 when e is 0).
 * An output texel is the mean of taps x taps bilinear samples of the panorama at the directions of a regular grid over its square,
 * at most 65504: a finite half whatever the file holds. The same rule in plain serial C++ is ur_host_env_panorama (include/ur_host.h).
 */
#ifndef UR_ENV_PANORAMA_H
#define UR_ENV_PANORAMA_H

#include <stddef.h>
#include <stdint.h>

#include "ur_hotpath.h"

#ifdef __cplusplus
extern "C" {
#endif

#define UR_ENV_PANORAMA_MAX_WIDTH 16384u
#define UR_ENV_PANORAMA_MAX_HEIGHT 8192u
#define UR_ENV_PANORAMA_MAX_BASE_SIZE 2048u
#define UR_ENV_PANORAMA_MAX_TAPS 16u
/* ur_env_panorama puts at most this many operations on the context's stream, whatever the sizes: one launch. */
#define UR_ENV_PANORAMA_MAX_STREAM_OPS 1u

/* Builds the six faces on the context's stream: asynchronous, no host allocation, no copy, no scratch, the host reads no device memory
 * and does not synchronise; at most UR_ENV_PANORAMA_MAX_STREAM_OPS stream operations.
 * Device memory: rgbe_device (rgbe_bytes = 4 * width * height, 4-byte aligned, only read), dst_device (dst_bytes = 6 * base_size^2 * 8,
 * 16-byte aligned: every byte is written, so what it holds on entry does not matter). taps: the sub-samples a side of an output texel,
 * a power of two 1..UR_ENV_PANORAMA_MAX_TAPS; ur_host_env_panorama_taps (include/ur_host.h) recommends one.
 * UR_EINVAL (ur_last_error has the text), decided from the arguments alone, nothing launched: a null context or pointer; a width outside
 * 1..UR_ENV_PANORAMA_MAX_WIDTH or a height outside 1..UR_ENV_PANORAMA_MAX_HEIGHT; a base_size that is no power of two or above
 * UR_ENV_PANORAMA_MAX_BASE_SIZE; taps that is no power of two in 1..16; rgbe_bytes or dst_bytes that are not the panorama's and the
 * cube's; a source that is not 4-byte aligned or a destination that is not 16-byte aligned; source and destination overlapping. */
int ur_env_panorama(ur_ctx* ctx, const void* rgbe_device, size_t rgbe_bytes, uint32_t width, uint32_t height, uint32_t base_size, uint32_t taps,
                    void* dst_device, size_t dst_bytes);

#ifdef __cplusplus
}
#endif
#endif /* UR_ENV_PANORAMA_H */
