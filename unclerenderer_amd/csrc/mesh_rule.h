// The mesh rule, once, for the kernels (csrc/mesh_build.hip) and the serial host build (csrc/mesh_host.cpp):
// the arithmetic, the per-triangle and per-vertex steps of FMesh::GenerateNormalsIfMissing / GenerateTangentsIfMissing
// (Mesh.cpp:190-331), the vertex assembly and index expansion of GltfLoader.cpp:811-999, and the host-only checks and layout of
// include/ur_mesh.h. No HIP in it beyond the function qualifiers: the plain host compiler builds it.
// All arithmetic is uncontracted fp32 (the units that include this are built with -ffp-contract=off).
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/ur_mesh.h"

#if defined(__HIPCC__)
#define UR_MESH_HD __host__ __device__ inline
#else
#define UR_MESH_HD inline
#endif

namespace ur_mesh {

struct F3 { float x, y, z; };
struct F4 { float x, y, z, w; };

UR_MESH_HD float dot3(F3 a, F3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
UR_MESH_HD F3 sub(F3 a, F3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
UR_MESH_HD F3 add(F3 a, F3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
UR_MESH_HD F3 scale(F3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
UR_MESH_HD F3 cross(F3 a, F3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
// v / sqrt(dot3(v, v)): (0, 0, 0) for a zero length, NaN for an infinite one
UR_MESH_HD F3 normalize(F3 v)
{
    const float length = sqrtf(dot3(v, v));
    if (length == 0.0f) return {0.0f, 0.0f, 0.0f};
    if (length == INFINITY) { const float q = NAN; return {q, q, q}; }
    return {v.x / length, v.y / length, v.z / length};
}

UR_MESH_HD bool normal_valid(F3 n) { return dot3(n, n) > 1e-6f; }   // IsNormalValid
UR_MESH_HD bool tangent_valid(F3 t) { return dot3(t, t) > 1e-6f; }  // IsTangentValid (xyz alone)

// --- per triangle ---
UR_MESH_HD F3 face_normal(F3 p0, F3 p1, F3 p2) { return cross(sub(p1, p0), sub(p2, p0)); }
// false: the triangle is skipped (|det| < 1e-8; a NaN determinant is not skipped)
UR_MESH_HD bool face_tangent(F3 p0, F3 p1, F3 p2, float u0, float v0, float u1, float v1, float u2, float v2, F3& tangent, F3& bitangent)
{
    const F3 e1 = sub(p1, p0), e2 = sub(p2, p0);
    const float d1x = u1 - u0, d1y = v1 - v0, d2x = u2 - u0, d2y = v2 - v0;
    const float det = d1x * d2y - d1y * d2x;
    if (fabsf(det) < 1e-8f) { tangent = {0.0f, 0.0f, 0.0f}; bitangent = {0.0f, 0.0f, 0.0f}; return false; }
    const float inv = 1.0f / det;
    tangent = scale(sub(scale(e1, d2y), scale(e2, d1y)), inv);
    bitangent = scale(sub(scale(e2, d1x), scale(e1, d2x)), inv);
    return true;
}

// --- per vertex ---
UR_MESH_HD F3 unit_or_z(F3 n)
{
    if (dot3(n, n) <= 1e-8f) n = {0.0f, 0.0f, 1.0f};
    return normalize(n);
}
UR_MESH_HD F3 finish_normal(F3 sum) { return unit_or_z(sum); }
// `normal` is the vertex's normal as the normal pass left it
UR_MESH_HD F4 finish_tangent(F3 normal, F3 tangent, F3 bitangent)
{
    const F3 n = unit_or_z(normal);
    if (dot3(tangent, tangent) <= 1e-8f || dot3(bitangent, bitangent) <= 1e-8f) {
        const F3 up = fabsf(n.x) < 0.99f ? F3{0.0f, 1.0f, 0.0f} : F3{1.0f, 0.0f, 0.0f}; // BuildOrthonormalTangent
        const F3 t = normalize(cross(up, n));
        return {t.x, t.y, t.z, 1.0f};
    }
    const F3 t = normalize(sub(tangent, scale(n, dot3(n, tangent))));
    const F3 b = normalize(bitangent);
    const float handedness = dot3(cross(n, t), b) < 0.0f ? -1.0f : 1.0f;
    return {t.x, t.y, t.z, handedness};
}

// --- bounds (RendererUtils.cpp:72-79) from min and max ---
UR_MESH_HD void finish_bounds(ur_mesh_info& info)
{
    for (int k = 0; k < 3; ++k) info.center[k] = 0.5f * (info.min[k] + info.max[k]);
    const F3 extent = {info.max[0] - info.min[0], info.max[1] - info.min[1], info.max[2] - info.min[2]};
    const float radius = sqrtf(dot3(extent, extent)) * 0.5f;
    info.radius = radius < 1.0f ? 1.0f : radius; // std::max(radius, 1.0f): a NaN stays
}

// --- layout ---
// a primitive and where it lies in the mesh: what the kernels read
struct Prim {
    ur_mesh_primitive p;
    uint32_t vertex_offset, index_start, index_count, pad;
};

UR_MESH_HD uint32_t index_bytes(uint32_t component_type) { return component_type == UR_MESH_INDEX_U8 ? 1u : component_type == UR_MESH_INDEX_U16 ? 2u : 4u; }
// the position in the primitive's raw indices that output index j of the primitive is taken from (GltfLoader.cpp:935-989)
UR_MESH_HD uint32_t raw_position(uint32_t mode, uint32_t j)
{
    if (mode == UR_MESH_MODE_TRIANGLES) return j;
    const uint32_t t = j / 3u, c = j - 3u * t, i = t + 2u;
    if (mode == UR_MESH_MODE_TRIANGLE_FAN) return c == 0u ? 0u : i - 2u + c;
    if (c == 2u) return i; // strip: (i - 2, i - 1, i), the first two exchanged when i is odd
    return i - 2u + ((i & 1u) ? 1u - c : c);
}
// (every fp32 and u32 of the buffer is 4-byte aligned: ur_mesh_build's checks; the host build takes a buffer at any address)
UR_MESH_HD uint32_t load_u32(const uint8_t* at)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return *reinterpret_cast<const uint32_t*>(at);
#else
    uint32_t v;
    memcpy(&v, at, 4);
    return v;
#endif
}
UR_MESH_HD uint32_t raw_index(const uint8_t* buffer, const ur_mesh_primitive& p, uint32_t position)
{
    const uint8_t* at = buffer + p.index_offset + (uint64_t)position * index_bytes(p.index_component_type);
    if (p.index_component_type == UR_MESH_INDEX_U8) return at[0];
    if (p.index_component_type == UR_MESH_INDEX_U16) return (uint32_t)at[0] | ((uint32_t)at[1] << 8);
    return load_u32(at);
}

// the 16 words of vertex i of a primitive (GltfLoader.cpp:811-892): floats are copied as bits, a negation flips the sign bit
UR_MESH_HD void assemble_vertex(const uint8_t* buffer, const ur_mesh_primitive& p, uint32_t i, uint32_t w[16])
{
    const uint32_t kSign = 0x80000000u, kOne = 0x3F800000u;
    const uint8_t* at = buffer + p.position.offset + (uint64_t)i * p.position.stride;
    w[0] = load_u32(at); w[1] = load_u32(at + 4); w[2] = load_u32(at + 8) ^ kSign;
    if (p.normal.present) {
        at = buffer + p.normal.offset + (uint64_t)i * p.normal.stride;
        w[3] = load_u32(at); w[4] = load_u32(at + 4); w[5] = load_u32(at + 8) ^ kSign;
    } else { w[3] = 0u; w[4] = 0u; w[5] = kOne ^ kSign; }
    if (p.texcoord.present) {
        at = buffer + p.texcoord.offset + (uint64_t)i * p.texcoord.stride;
        w[6] = load_u32(at); w[7] = load_u32(at + 4);
    } else { w[6] = 0u; w[7] = 0u; }
    if (p.tangent.present) {
        at = buffer + p.tangent.offset + (uint64_t)i * p.tangent.stride;
        w[8] = load_u32(at); w[9] = load_u32(at + 4); w[10] = load_u32(at + 8) ^ kSign; w[11] = load_u32(at + 12) ^ kSign;
    } else { w[8] = 0u; w[9] = 0u; w[10] = kSign; w[11] = kOne ^ kSign; }
    w[12] = w[13] = w[14] = w[15] = kOne;
    if (p.color.present) {
        at = buffer + p.color.offset + (uint64_t)i * p.color.stride;
        w[12] = load_u32(at); w[13] = load_u32(at + 4); w[14] = load_u32(at + 8);
        if (p.color_components == 4u) w[15] = load_u32(at + 12);
    }
}
UR_MESH_HD float as_float(uint32_t bits)
{
    float f;
    __builtin_memcpy(&f, &bits, 4);
    return f;
}

// the scan's tile in vertices, the longest segment a lane sums on its own, the bytes of the scratch's header
constexpr uint32_t kScanTile = 1024u, kLaneSegment = 32u, kHeaderBytes = 256u;

// Host only. The checks of include/ur_mesh.h over the primitives, and the layout; nullptr, or the refusal's text (in `text`).
// prims: n entries filled in, or nullptr.
inline const char* check_stream(const char* who, uint32_t k, const char* name, const ur_mesh_stream& s, uint32_t floats, uint32_t count, uint64_t buffer_size, char* text,
                                size_t cap)
{
    if (!s.present) return nullptr;
    if (s.stride == 0u || s.stride % 4u != 0u) { snprintf(text, cap, "%s: primitive %u: %s stride %u (a multiple of 4, not 0)", who, k, name, s.stride); return text; }
    if (s.offset % 4u != 0u) { snprintf(text, cap, "%s: primitive %u: %s offset %llu is not 4-byte aligned", who, k, name, (unsigned long long)s.offset); return text; }
    const uint64_t span = (uint64_t)(count - 1u) * s.stride + 4u * floats;
    if (s.offset > buffer_size || span > buffer_size - s.offset) {
        snprintf(text, cap, "%s: primitive %u: %s reads past the buffer (offset %llu, stride %u, %u elements, buffer %llu bytes)", who, k, name,
                 (unsigned long long)s.offset, s.stride, count, (unsigned long long)buffer_size);
        return text;
    }
    return nullptr;
}

inline uint64_t align16(uint64_t v) { return (v + 15u) & ~(uint64_t)15u; }

// scratch: byte offsets of the parts (csrc/mesh_build.hip), each 16-byte aligned
struct Scratch { uint64_t table, counts, sums, corners, queue, normals, tangents, skips, total; };
inline Scratch scratch_layout(uint32_t n, uint64_t vertices, uint64_t indices)
{
    Scratch s{};
    const uint64_t triangles = indices / 3u;
    s.table = kHeaderBytes;
    s.counts = s.table + align16((uint64_t)n * sizeof(Prim));
    s.sums = s.counts + align16(4u * vertices);
    s.corners = s.sums + align16(4u * ((vertices + kScanTile - 1u) / kScanTile));
    s.queue = s.corners + align16(4u * indices);
    s.normals = s.queue + align16(4u * (indices / (kLaneSegment + 1u) + 1u));
    s.tangents = s.normals + align16(12u * triangles);
    s.skips = s.tangents + align16(24u * triangles);
    s.total = s.skips + align16(triangles);
    return s;
}

inline const char* check_primitives(const char* who, const ur_mesh_primitive* primitives, uint32_t n, uint64_t buffer_size, ur_mesh_layout* layout, Prim* prims,
                                    ur_mesh_section* sections, char* text, size_t cap)
{
    if (!primitives || n == 0u) { snprintf(text, cap, "%s: no primitives", who); return text; }
    uint64_t vertices = 0u, indices = 0u;
    for (uint32_t k = 0u; k < n; ++k) {
        const ur_mesh_primitive& p = primitives[k];
        if (p.mode != UR_MESH_MODE_TRIANGLES && p.mode != UR_MESH_MODE_TRIANGLE_STRIP && p.mode != UR_MESH_MODE_TRIANGLE_FAN) {
            snprintf(text, cap, "%s: primitive %u: mode %u (4 triangles, 5 strip, 6 fan)", who, k, p.mode); return text;
        }
        if (p.index_component_type != UR_MESH_INDEX_U8 && p.index_component_type != UR_MESH_INDEX_U16 && p.index_component_type != UR_MESH_INDEX_U32) {
            snprintf(text, cap, "%s: primitive %u: index component type %u (5121, 5123, 5125)", who, k, p.index_component_type); return text;
        }
        if (p.vertex_count == 0u) { snprintf(text, cap, "%s: primitive %u: no vertices", who, k); return text; }
        if (p.index_count < 3u) { snprintf(text, cap, "%s: primitive %u: %u indices (at least 3)", who, k, p.index_count); return text; }
        if (p.mode == UR_MESH_MODE_TRIANGLES && p.index_count % 3u != 0u) {
            snprintf(text, cap, "%s: primitive %u: a triangle list of %u indices (a multiple of 3)", who, k, p.index_count); return text;
        }
        if (!p.position.present) { snprintf(text, cap, "%s: primitive %u: no POSITION", who, k); return text; }
        if (p.color.present && p.color_components != 3u && p.color_components != 4u) {
            snprintf(text, cap, "%s: primitive %u: a colour of %u components (3 or 4)", who, k, p.color_components); return text;
        }
        const char* bad = check_stream(who, k, "POSITION", p.position, 3u, p.vertex_count, buffer_size, text, cap);
        if (!bad) bad = check_stream(who, k, "NORMAL", p.normal, 3u, p.vertex_count, buffer_size, text, cap);
        if (!bad) bad = check_stream(who, k, "TEXCOORD_0", p.texcoord, 2u, p.vertex_count, buffer_size, text, cap);
        if (!bad) bad = check_stream(who, k, "TANGENT", p.tangent, 4u, p.vertex_count, buffer_size, text, cap);
        if (!bad) bad = check_stream(who, k, "COLOR_0", p.color, p.color_components, p.vertex_count, buffer_size, text, cap);
        if (bad) return bad;
        const uint32_t size = index_bytes(p.index_component_type);
        if (p.index_offset % size != 0u) {
            snprintf(text, cap, "%s: primitive %u: index offset %llu is not %u-byte aligned", who, k, (unsigned long long)p.index_offset, size); return text;
        }
        if (p.index_offset > buffer_size || (uint64_t)p.index_count * size > buffer_size - p.index_offset) {
            snprintf(text, cap, "%s: primitive %u: the indices read past the buffer (offset %llu, %u of %u bytes, buffer %llu bytes)", who, k,
                     (unsigned long long)p.index_offset, p.index_count, size, (unsigned long long)buffer_size);
            return text;
        }
        const uint64_t out = p.mode == UR_MESH_MODE_TRIANGLES ? (uint64_t)p.index_count : 3u * ((uint64_t)p.index_count - 2u);
        if (vertices + p.vertex_count > 0xFFFFFFFFull || indices + out > 0xFFFFFFFFull) {
            snprintf(text, cap, "%s: more than 2^32 - 1 vertices or indices at primitive %u", who, k); return text;
        }
        if (prims) { prims[k].p = p; prims[k].vertex_offset = (uint32_t)vertices; prims[k].index_start = (uint32_t)indices; prims[k].index_count = (uint32_t)out; prims[k].pad = 0u; }
        if (sections) sections[k] = {(uint32_t)vertices, (uint32_t)indices, (uint32_t)out};
        vertices += p.vertex_count;
        indices += out;
    }
    if (layout) {
        layout->vertex_count = (uint32_t)vertices;
        layout->index_count = (uint32_t)indices;
        layout->scratch_bytes = scratch_layout(n, vertices, indices).total;
    }
    return nullptr;
}

} // namespace ur_mesh
