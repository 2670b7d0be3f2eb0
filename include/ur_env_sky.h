/*
 * ur_env_sky.h - the sky capture: the procedural sky the frame draws behind the geometry (ur_sky_atmosphere, SkyAtmosphere.hlsl:60-94)
 * becomes the top level of an HDR cube - six square R16G16B16A16_FLOAT faces of a power-of-two edge, face-major, alpha 1.0 - on the device,
 * in one asynchronous call with nothing read back. The result is exactly the source of ur_env_prefilter
 * (include/ur_env_prefilter.h) and the layout ur_env_panorama (include/ur_env_panorama.h) writes:
 *     ur_sky_constants -> ur_env_sky -> ur_env_prefilter -> ur_env_cube_build -> Lighting / Forward,
 * so reflections and ambient light follow LightDirection and LightColor; call it again whenever the sun moves. An output texel is the
 * mean of taps x taps evaluations of the sky at the directions of a regular grid over its square, at most 65504. There is no sun disk.
 * The same rule in plain serial C++ is ur_host_env_sky (include/ur_host.h).
 */
#ifndef UR_ENV_SKY_H
#define UR_ENV_SKY_H

#include <stddef.h>
#include <stdint.h>

#include "ur_hotpath.h"

#ifdef __cplusplus
extern "C" {
#endif

#define UR_ENV_SKY_MAX_BASE_SIZE 2048u
#define UR_ENV_SKY_MAX_TAPS 16u
/* ur_env_sky puts at most this many operations on the context's stream, whatever the sizes: one launch. */
#define UR_ENV_SKY_MAX_STREAM_OPS 1u

/* Builds the six faces on the context's stream: asynchronous, no host allocation, no copy, no scratch, the host reads no device memory
 * and does not synchronise; at most UR_ENV_SKY_MAX_STREAM_OPS stream operations. Of `sky` only CameraPosition[1], LightDirection and
 * LightColor are read, before the call returns (a capture has no camera: the matrices are ignored); ur_host_env_sky_params
 * (include/ur_host.h) gives the values they are folded to. Device memory: dst_device (dst_bytes = 6 * base_size^2 * 8, 16-byte aligned:
 * every byte is written, so what it holds on entry does not matter). taps: the sub-samples a side of an output texel, a power of two
 * 1..UR_ENV_SKY_MAX_TAPS; the sky is smooth, 1 is the texel centre's value and what the frame's sky pass would draw there.
 * UR_EINVAL (ur_last_error has the text), decided from the arguments alone, nothing launched: a null context or pointer; a base_size
 * that is no power of two or above UR_ENV_SKY_MAX_BASE_SIZE; taps that is no power of two in 1..16; dst_bytes that is not the cube's; a
 * destination that is not 16-byte aligned; a CameraPosition[1], LightDirection or LightColor that is not finite; a LightDirection of
 * length zero. */
int ur_env_sky(ur_ctx* ctx, const ur_sky_constants* sky, uint32_t base_size, uint32_t taps, void* dst_device, size_t dst_bytes);

#ifdef __cplusplus
}
#endif
#endif /* UR_ENV_SKY_H */
