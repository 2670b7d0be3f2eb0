// ur_host_scene_build (include/ur_host.h): the scene rule of DESIGN.md section 3.18 in plain serial C++, draw by draw in command order,
// over csrc/scene_rule.h, the functions the kernels of csrc/scene_build.hip run. Any compiler builds it; it is the CPU fallback and the
// time baseline of the device build.

#include "../../include/ur_host.h"
#include "scene_rule.h"

extern "C" int ur_host_scene_build(const ur_scene_build_tables* tables, const ur_scene_constants* frame, const ur_scene_build_outputs* outputs,
                                   uint64_t constants_address, uint32_t flags)
{
    using namespace ur_scene;
    char text[256];
    if (check_tables("ur_host_scene_build", tables, frame, outputs, flags, text, sizeof text)) return UR_EINVAL;
    const ur_scene_build_tables& t = *tables;
    const ur_scene_build_outputs& o = *outputs;
    const bool full = (flags & UR_SCENE_BUILD_TRANSFORMS_ONLY) == 0u;
    uint32_t tmpl[4u * kConstantsPieces];
    memcpy(tmpl, frame, kConstantsBytes);
    uint8_t* commands = static_cast<uint8_t*>(o.commands);
    uint8_t* constants = static_cast<uint8_t*>(o.constants);

    Box box = empty_box();
    uint32_t skipped = 0u;
    for (uint32_t i = 0u; i < t.draw_count; ++i) {
        const ur_scene_draw d = t.draws[i];
        if (!draw_in_range(d, t.node_count, t.mesh_count, t.material_count, o.slot_count)) {
            ++skipped;
            memset(&o.bounds[2u * (size_t)i], 0, 2u * sizeof(ur_float4));
            if (o.centers) memset(&o.centers[i], 0, sizeof(ur_float4));
            if (full) memset(commands + 64u * (size_t)i, 0, 64u);
            continue;
        }
        const Placed p = place(t.nodes[d.node], t.mesh_infos[d.mesh]);
        o.bounds[2u * (size_t)i] = ur_float4{p.bounds_min[0], p.bounds_min[1], p.bounds_min[2], 0.0f};
        o.bounds[2u * (size_t)i + 1u] = ur_float4{p.bounds_max[0], p.bounds_max[1], p.bounds_max[2], 0.0f};
        if (o.centers) o.centers[i] = ur_float4{p.center[0], p.center[1], p.center[2], p.radius};
        box_add(box, p.center, p.radius);
        const uint64_t offset = (uint64_t)d.constants_slot * o.constants_stride;
        uint8_t* record = constants + offset;
        memcpy(record, p.world.m, 64u);
        if (!full) continue;
        uint32_t factors[4u * kFactorPieces];
        memcpy(factors, &t.materials[d.material], sizeof factors);
        for (uint32_t piece = 4u; piece < kConstantsPieces; ++piece) {
            uint32_t w[4];
            constants_piece(piece, tmpl + 4u * piece, factors, d.object_id, w);
            memcpy(record + 16u * piece, w, 16u);
        }
        uint32_t w[16];
        command_words(t.meshes[d.mesh], d, constants_address + offset, w);
        memcpy(commands + 64u * (size_t)i, w, 64u);
    }
    ur_scene_build_summary s;
    finish_summary(box, t.draw_count, skipped, s);
    *o.summary = s;
    return UR_OK;
}
