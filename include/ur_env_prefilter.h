/*
 * ur_env_prefilter.h - environment prefilter: the top level of an HDR cube - six square R16G16B16A16_FLOAT faces of a power-of-two edge,
 * face-major - becomes the full prefiltered chain that Shaders/DeferredLighting.hlsl and Shaders/ForwardPS.hlsl expect of an environment
 * cube: level k of L = log2(base_size) + 1 holds the environment filtered for roughness k / (L - 1) (GGX, alpha = roughness^2, V = N),
 * down to the 1 x 1 level the shaders read as irradiance. On the device, in one asynchronous call with nothing read back (DESIGN.md
 * section 3.20). The result is an RGBA16F payload in DDS order, face-major with mips inner: what
 * ur_env_cube_build(..., UR_ENV_SOURCE_RGBA16F, base_size, L, ...) (include/ur_env_cube.h) stages. The same rule in plain serial C++ is
 * ur_host_env_prefilter, the sample table comes from ur_host_env_prefilter_table (include/ur_host.h).
 * Finite source texels are the contract. A texel that is not finite changes no address: directions and levels come from the table alone.
 */
#ifndef UR_ENV_PREFILTER_H
#define UR_ENV_PREFILTER_H

#include <stddef.h>
#include <stdint.h>

#include "ur_env_cube.h"

#ifdef __cplusplus
extern "C" {
#endif

#define UR_ENV_PREFILTER_MAX_BASE_SIZE 2048u
#define UR_ENV_PREFILTER_MIN_SAMPLES 16u
#define UR_ENV_PREFILTER_MAX_SAMPLES 4096u
/* ur_env_prefilter puts at most this many operations on the context's stream, whatever the base size: the top level (1), the source
 * pyramid (a launch a level, at most 11), its bordered faces (2) and the filter (1). */
#define UR_ENV_PREFILTER_MAX_STREAM_OPS 15u

/* Bytes of the sample table of a cube of edge base_size filtered with sample_count samples a texel: 16 L + 16 sample_count (L - 1).
 * 0 for a base_size that is no power of two or above UR_ENV_PREFILTER_MAX_BASE_SIZE, or a sample_count that is no power of two in
 * UR_ENV_PREFILTER_MIN_SAMPLES .. UR_ENV_PREFILTER_MAX_SAMPLES. Host only. */
size_t ur_env_prefilter_table_bytes(uint32_t base_size, uint32_t sample_count);
/* Bytes of device scratch a call needs: the source pyramid and its bordered faces. 0 for a base_size the call refuses. Host only. */
size_t ur_env_prefilter_scratch_bytes(uint32_t base_size);

/* Filters the chain on the context's stream: asynchronous, no host allocation, no copy, the host reads no device memory and does not
 * synchronise; at most UR_ENV_PREFILTER_MAX_STREAM_OPS stream operations.
 * Device memory, each 16-byte aligned: src_device (src_bytes = 6 * base_size^2 * 8, only read), table_device (at least
 * ur_env_prefilter_table_bytes(base_size, sample_count) bytes that ur_host_env_prefilter_table wrote for the same two numbers, only read),
 * dst_device (dst_bytes = ur_env_cube_source_bytes(UR_ENV_SOURCE_RGBA16F, base_size, L): every byte is written, so what it holds on
 * entry does not matter), scratch (at least ur_env_prefilter_scratch_bytes(base_size) bytes; what it holds on entry does not matter and
 * what it holds afterwards is unspecified).
 * UR_EINVAL (ur_last_error has the text), decided from the arguments alone, nothing launched: a null context or pointer; a base_size
 * that is no power of two or above UR_ENV_PREFILTER_MAX_BASE_SIZE; a sample_count that is no power of two or out of range; src_bytes or
 * dst_bytes that are not the cube's; a short table or scratch; a pointer that is not 16-byte aligned; any two of source, table,
 * destination and scratch overlapping. */
int ur_env_prefilter(ur_ctx* ctx, const void* src_device, size_t src_bytes, uint32_t base_size, uint32_t sample_count, const void* table_device,
                     size_t table_bytes, void* dst_device, size_t dst_bytes, void* scratch, size_t scratch_bytes);

#ifdef __cplusplus
}
#endif
#endif /* UR_ENV_PREFILTER_H */
