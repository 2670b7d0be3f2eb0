/*
 * ur_scene.h — scene -> instance AABB extraction, host only: scene JSON + glTF JSON in, the cull
 * pass's ModelBounds order and boxes out. See csrc/scene.cpp for the reference citations and the two stated differences
 * (accessor min/max instead of scanning the .bin; deterministic order inside a pipeline-key group).
 */
#ifndef UR_SCENE_H
#define UR_SCENE_H

#include <stdint.h>

#include "ur_scene_build.h"

#ifdef __cplusplus
extern "C" {
#endif

#define UR_SCENE_OK 0
#define UR_SCENE_EINVAL (-1)
#define UR_SCENE_EJSON (-2)     /* malformed JSON */
#define UR_SCENE_EEMPTY (-3)    /* no models / no renderable meshes */
#define UR_SCENE_ENOBOUNDS (-4) /* a POSITION accessor lacks min/max */
#define UR_SCENE_ECAPACITY (-5)

/* One draw command's worth of FSceneModelResource (RendererUtils.h:113-…): what the cull pass and the light set-up use. */
typedef struct ur_scene_model {
    float bounds_min[3];
    float bounds_max[3];
    float center[3];        /* mesh-box centre through World */
    float radius;           /* mesh radius x max model scale x max node scale */
    uint32_t pipeline_key;  /* BuildPipelineKey, DeferredRenderer.cpp:28-36 */
    uint32_t material_index;
    uint32_t model_index, node_order, mesh_index, primitive_index;
} ur_scene_model;

typedef struct ur_scene_summary {
    uint32_t model_count;
    float scene_center[3];
    float scene_radius;
} ur_scene_summary;

/* Number of entries of the scene JSON's "models" array (-1 on malformed JSON). */
int ur_scene_model_count(const char* scene_json);
/* The i-th model's "path" (relative to the assets root), NUL-terminated into buf; returns its length or -1. */
int ur_scene_model_path(const char* scene_json, uint32_t index, char* buf, uint32_t cap);
/* scene_json: text of Assets/Scenes/<x>.json. gltf_json[i]: text of the i-th model's .gltf (JSON form).
 * out (nullable, capacity entries): models in command order. summary (nullable): count + scene centre/radius. */
int ur_scene_extract(const char* scene_json, const char* const* gltf_json, uint32_t gltf_count, ur_scene_model* out, uint32_t capacity,
                     ur_scene_summary* summary);

/* One draw of the plan, in ur_scene_extract's command order: what ur_scene_build's draw table (include/ur_scene_build.h) is made of. */
typedef struct ur_scene_plan_draw {
    uint32_t node;           /* index into the plan's node records */
    uint32_t mesh;           /* mesh_base[model_index] + the glTF mesh index: the mesh among all models' meshes */
    uint32_t primitive;      /* the mesh's primitive (section) */
    uint32_t material_index; /* glTF material index of the model's file, 0xFFFFFFFF: none */
    uint32_t pipeline_key;
    uint32_t model_index;
    uint32_t constants_slot; /* the draw's place in creation order (model, node, primitive), before the sort */
    uint32_t object_id;      /* creation order + 1 (RendererUtils.cpp:306,485) */
} ur_scene_plan_draw;

/* The same walk as ur_scene_extract, for ur_scene_build: the node records (one per placed glTF node, in creation order: node_world is the
 * node's left-handed world matrix, scale / rotation / translate the model's "scale", "rotate_euler" as XMMatrixRotationRollPitchYaw and
 * "translate") and the draws in ur_scene_extract's stable order. mesh_base: gltf_count entries, the number of meshes of the models in
 * front. nodes / draws (nullable) take node_capacity / draw_capacity records; *node_count and *draw_count are always written.
 * UR_SCENE_EINVAL for a null mesh_base or count pointer; otherwise ur_scene_extract's codes. */
int ur_scene_plan(const char* scene_json, const char* const* gltf_json, uint32_t gltf_count, const uint32_t* mesh_base, ur_scene_node* nodes,
                  uint32_t node_capacity, uint32_t* node_count, ur_scene_plan_draw* draws, uint32_t draw_capacity, uint32_t* draw_count);

#ifdef __cplusplus
}
#endif
#endif /* UR_SCENE_H */
