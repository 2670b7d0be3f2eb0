// ur_host_mesh_build (include/ur_host.h): the mesh rule of DESIGN.md section 3.17 in plain serial C++, in the reference's own order -
// assemble, expand, the normal pass, the tangent pass, the bounds - over csrc/mesh_rule.h, the per-triangle and per-vertex functions
// the kernels of csrc/mesh_build.hip run. Any compiler builds it; it is the CPU fallback and the time baseline of the device build.

#include <vector>

#include "../../include/ur_host.h"
#include "mesh_rule.h"

namespace {

using namespace ur_mesh;

struct Vertex { float f[16]; };

F3 position(const Vertex& v) { return {v.f[0], v.f[1], v.f[2]}; }

} // namespace

extern "C" int ur_host_mesh_build(const void* buffer, uint64_t buffer_size, const ur_mesh_primitive* primitives, uint32_t n, void* vertices_out, uint32_t* indices_out,
                                  ur_mesh_section* sections_out, ur_mesh_info* info_out)
{
    if (!buffer || !vertices_out || !indices_out || !info_out) return UR_EINVAL;
    char text[256];
    ur_mesh_layout layout{};
    std::vector<Prim> prims(n ? n : 1u);
    if (check_primitives("ur_host_mesh_build", primitives, n, buffer_size, &layout, prims.data(), sections_out, text, sizeof text)) return UR_EINVAL;
    const uint8_t* bytes = static_cast<const uint8_t*>(buffer);
    const size_t V = layout.vertex_count, I = layout.index_count;
    std::vector<Vertex> vertices(V);
    for (const Prim& prim : prims) {
        for (uint32_t i = 0u; i < prim.p.vertex_count; ++i) {
            uint32_t w[16];
            assemble_vertex(bytes, prim.p, i, w);
            memcpy(vertices[prim.vertex_offset + i].f, w, 64);
        }
        for (uint32_t j = 0u; j < prim.index_count; ++j)
            indices_out[prim.index_start + j] = raw_index(bytes, prim.p, raw_position(prim.p.mode, j)) + prim.vertex_offset;
    }

    ur_mesh_info info{};
    for (size_t t = 0u; t + 2u < I; t += 3u)
        if (indices_out[t] >= V || indices_out[t + 1u] >= V || indices_out[t + 2u] >= V) ++info.out_of_range_triangles;

    bool normals_valid = true, tangents_valid = true;
    for (const Vertex& v : vertices) normals_valid = normals_valid && normal_valid({v.f[3], v.f[4], v.f[5]});
    if (!normals_valid) {
        info.normals_regenerated = 1u;
        std::vector<F3> sum(V, F3{0.0f, 0.0f, 0.0f});
        for (size_t t = 0u; t + 2u < I; t += 3u) {
            const uint32_t i0 = indices_out[t], i1 = indices_out[t + 1u], i2 = indices_out[t + 2u];
            if (i0 >= V || i1 >= V || i2 >= V) continue;
            const F3 face = face_normal(position(vertices[i0]), position(vertices[i1]), position(vertices[i2]));
            sum[i0] = add(sum[i0], face);
            sum[i1] = add(sum[i1], face);
            sum[i2] = add(sum[i2], face);
        }
        for (size_t v = 0u; v < V; ++v) {
            const F3 normal = finish_normal(sum[v]);
            vertices[v].f[3] = normal.x; vertices[v].f[4] = normal.y; vertices[v].f[5] = normal.z;
        }
    }
    for (const Vertex& v : vertices) tangents_valid = tangents_valid && tangent_valid({v.f[8], v.f[9], v.f[10]});
    if (!tangents_valid) {
        info.tangents_regenerated = 1u;
        std::vector<F3> tangent_sum(V, F3{0.0f, 0.0f, 0.0f}), bitangent_sum(V, F3{0.0f, 0.0f, 0.0f});
        for (size_t t = 0u; t + 2u < I; t += 3u) {
            const uint32_t i0 = indices_out[t], i1 = indices_out[t + 1u], i2 = indices_out[t + 2u];
            if (i0 >= V || i1 >= V || i2 >= V) continue;
            const Vertex &a = vertices[i0], &b = vertices[i1], &c = vertices[i2];
            F3 tangent, bitangent;
            if (!face_tangent(position(a), position(b), position(c), a.f[6], a.f[7], b.f[6], b.f[7], c.f[6], c.f[7], tangent, bitangent)) {
                ++info.skipped_determinant_triangles;
                continue;
            }
            tangent_sum[i0] = add(tangent_sum[i0], tangent);
            tangent_sum[i1] = add(tangent_sum[i1], tangent);
            tangent_sum[i2] = add(tangent_sum[i2], tangent);
            bitangent_sum[i0] = add(bitangent_sum[i0], bitangent);
            bitangent_sum[i1] = add(bitangent_sum[i1], bitangent);
            bitangent_sum[i2] = add(bitangent_sum[i2], bitangent);
        }
        for (size_t v = 0u; v < V; ++v) {
            const F4 t = finish_tangent({vertices[v].f[3], vertices[v].f[4], vertices[v].f[5]}, tangent_sum[v], bitangent_sum[v]);
            vertices[v].f[8] = t.x; vertices[v].f[9] = t.y; vertices[v].f[10] = t.z; vertices[v].f[11] = t.w;
        }
    }

    for (int k = 0; k < 3; ++k) info.min[k] = info.max[k] = vertices[0].f[k];
    for (const Vertex& v : vertices)
        for (int k = 0; k < 3; ++k) {
            info.min[k] = v.f[k] < info.min[k] ? v.f[k] : info.min[k]; // std::min(Min, v)
            info.max[k] = info.max[k] < v.f[k] ? v.f[k] : info.max[k]; // std::max(Max, v)
        }
    finish_bounds(info);
    memcpy(vertices_out, vertices.data(), 64u * V);
    *info_out = info;
    return UR_OK;
}
