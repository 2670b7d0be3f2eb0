/*
 * ur_env_cube.h - environment cube build: the payload of a DDS cube - BC6H_UF16 / BC6H_SF16 blocks or R16G16B16A16_FLOAT texels, as it
 * lies in the file behind the header - becomes the staged IBL cube that ur_deferred_lighting, ur_deferred_lighting_sky and
 * ur_forward_pass sample (ur_lighting_tables::env_cube), on the device, in one asynchronous call with nothing read back (DESIGN.md
 * section 3.19). It writes what ur_stage_env_cube (include/ur_hotpath.h) writes for the same cube, to the byte: the bordered faces of
 * every mip, then the RGB row pairs. The same rule in plain serial C++ is ur_host_env_cube_build (include/ur_host.h).
 */
#ifndef UR_ENV_CUBE_H
#define UR_ENV_CUBE_H

#include <stddef.h>
#include <stdint.h>

#include "ur_hotpath.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the source formats, by their DXGI numbers */
#define UR_ENV_SOURCE_RGBA16F 10u
#define UR_ENV_SOURCE_BC6H_UF16 95u
#define UR_ENV_SOURCE_BC6H_SF16 96u
/* ur_env_cube_build puts at most this many operations on the context's stream, whatever the mip count: the decode launch, the border
 * launch and the row-pair launch. */
#define UR_ENV_CUBE_BUILD_MAX_STREAM_OPS 3u
#define UR_ENV_CUBE_MAX_BASE_SIZE 16384u /* the builds refuse a larger cube */

/* Bytes of a DDS cube payload: six faces, face-major with mips inner (the order ur_dds_decode_rgba16f walks). A level of edge
 * n = max(1, base_size >> m) is n * n texels of 8 bytes (RGBA16F) or ceil(n / 4)^2 blocks of 16 bytes (BC6H). 0 for base_size == 0,
 * mip_count == 0 or above 16, or an unknown format. Host only. */
size_t ur_env_cube_source_bytes(uint32_t format, uint32_t base_size, uint32_t mip_count);

/* Builds the staged cube on the context's stream: asynchronous, no host allocation, no copy, the host reads no device memory and does
 * not synchronise; at most UR_ENV_CUBE_BUILD_MAX_STREAM_OPS stream operations.
 * Device memory: src_device (src_bytes, 16-byte aligned, only read), dst_device (dst_texels units of 8 bytes, 16-byte aligned: every
 * byte is written, so what it holds on entry does not matter), info_device (one uint32_t, 4-byte aligned, or NULL: info_device[0]
 * receives the number of BC6H blocks of a reserved mode, which decode to (0, 0, 0, 1) as in D3D; 0 for RGBA16F. The call writes it, the
 * caller need not clear it).
 * UR_EINVAL (ur_last_error has the text), decided from the arguments alone, nothing launched: a null context, source or destination; an
 * unknown format; a cube ur_env_cube_texels refuses or base_size above UR_ENV_CUBE_MAX_BASE_SIZE;
 * src_bytes != ur_env_cube_source_bytes(format, base_size, mip_count); dst_texels != ur_env_cube_texels(base_size, mip_count); a source
 * or destination that is not 16-byte aligned, an info that is not 4-byte aligned; source, destination and info overlapping. */
int ur_env_cube_build(ur_ctx* ctx, const void* src_device, size_t src_bytes, uint32_t format, uint32_t base_size, uint32_t mip_count, ur_half4* dst_device,
                      size_t dst_texels, uint32_t* info_device);

#ifdef __cplusplus
}
#endif
#endif /* UR_ENV_CUBE_H */
