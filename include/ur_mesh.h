/*
 * ur_mesh.h - mesh build: the buffer of a glTF file (its .bin) becomes the 64-byte vertices and R32 indices the raster passes
 * draw (include/ur_raster.h), on the device, by the reference's rules: vertex assembly and index
 * expansion of GltfLoader.cpp:719-1028, FMesh::GenerateNormalsIfMissing and FMesh::GenerateTangentsIfMissing (Mesh.cpp:190-331),
 * the bounds of RendererUtils.cpp:46-82. One mesh is a glTF meshes[i]: its primitives in order, appended into one vertex array
 * and one index array. The same rule in plain serial C++ is ur_host_mesh_build (include/ur_host.h).
 */
#ifndef UR_MESH_H
#define UR_MESH_H

#include <stdint.h>

#include "ur_hotpath.h"

#ifdef __cplusplus
extern "C" {
#endif

#define UR_MESH_VERTEX_BYTES 64u /* POSITION at byte 0, NORMAL 12, TEXCOORD 24, TANGENT 32, COLOR 48 */
#define UR_MESH_MODE_TRIANGLES 4u
#define UR_MESH_MODE_TRIANGLE_STRIP 5u
#define UR_MESH_MODE_TRIANGLE_FAN 6u
#define UR_MESH_INDEX_U8 5121u
#define UR_MESH_INDEX_U16 5123u
#define UR_MESH_INDEX_U32 5125u
/* ur_mesh_build puts at most this many operations on the context's stream, whatever the mesh: one copy of the primitive table into
 * the scratch and 13 kernel launches. */
#define UR_MESH_BUILD_MAX_STREAM_OPS 14u

/* One attribute stream of fp32 values in the buffer: element i starts at byte offset + i * stride (the accessor's byteOffset plus the
 * view's; the view's byteStride or the packed size). offset and stride are multiples of 4, stride is not 0. present == 0: the stream
 * is absent, the other two fields are not looked at and the rule's default is assembled. */
typedef struct ur_mesh_stream {
    uint64_t offset;
    uint32_t stride;
    uint32_t present;
} ur_mesh_stream;

/* One glTF primitive. position is required. color_components is 3 (alpha 1) or 4 and looked at only when color is present.
 * index_component_type is UR_MESH_INDEX_*; index_offset is a multiple of the component's size; the indices are packed.
 * mode is UR_MESH_MODE_*. reserved is 0. */
typedef struct ur_mesh_primitive {
    ur_mesh_stream position, normal, texcoord, tangent, color;
    uint64_t index_offset;
    uint32_t index_count, index_component_type;
    uint32_t mode, vertex_count, color_components, reserved;
} ur_mesh_primitive; /* 112 bytes */

/* Where a primitive lies in the mesh: the vertices appended before it (already added to its indices), and its indices. */
typedef struct ur_mesh_section {
    uint32_t vertex_offset, index_start, index_count;
} ur_mesh_section;

typedef struct ur_mesh_layout {
    uint32_t vertex_count, index_count; /* V and I: 64 * V vertex bytes, 4 * I index bytes */
    uint64_t scratch_bytes;             /* what ur_mesh_build needs; the build clears what it reads */
} ur_mesh_layout;

/* What the build leaves on the device beside the geometry. The bounds are over the assembled positions; a coordinate of min / max is
 * NaN iff vertex 0's is. skipped_determinant_triangles is 0 unless tangents were regenerated. */
typedef struct ur_mesh_info {
    float min[3], max[3], center[3], radius;
    uint32_t normals_regenerated, tangents_regenerated;
    uint32_t skipped_determinant_triangles; /* |det| < 1e-8 in the tangent pass */
    uint32_t out_of_range_triangles;        /* an index >= V: the triangle adds to no sum; its indices are written as they are */
} ur_mesh_info; /* 56 bytes */

/* Host only: the layout of the mesh of primitives[0..n). sections: n entries, or NULL. UR_EINVAL (ur_last_error has the text) for a null
 * pointer, n == 0, a stream, present, that would read past buffer_size, a bad mode or component type, a triangle list whose count is not
 * a multiple of 3, fewer than 3 indices, a zero vertex count, a stride that is 0 or no multiple of 4, a misaligned offset, a colour of
 * neither 3 nor 4 components, or totals above 2^32 - 1. */
int ur_mesh_layout_of(const ur_mesh_primitive* primitives, uint32_t n, uint64_t buffer_size, ur_mesh_layout* out_layout, ur_mesh_section* sections);

/* Builds the mesh on the context's stream: asynchronous, the host reads nothing back and does not synchronise; at most
 * UR_MESH_BUILD_MAX_STREAM_OPS stream operations. `primitives` is host memory, read before the call returns.
 * Device memory: buffer (buffer_size bytes, 4-byte aligned, only read), vertices (64 * V bytes, 16-byte aligned), indices (4 * I bytes,
 * 4-byte aligned), scratch (scratch_bytes >= the layout's, 16-byte aligned, content on entry does not matter), info (one ur_mesh_info,
 * 4-byte aligned). UR_EINVAL for everything ur_mesh_layout_of refuses, a null or misaligned pointer, too little scratch, or outputs that
 * overlap each other, the scratch or the buffer: decided from the arguments alone, device memory is never read to decide. */
int ur_mesh_build(ur_ctx* ctx, const void* buffer, uint64_t buffer_size, const ur_mesh_primitive* primitives, uint32_t n, void* vertices, void* indices,
                  void* scratch, uint64_t scratch_bytes, ur_mesh_info* info);

#ifdef __cplusplus
}
#endif
#endif /* UR_MESH_H */
