"""Scene loading for the cull pass: Assets/Scenes/<x>.json + the models' .gltf JSON -> ModelBounds in command order.
The extraction itself is C++ (csrc/scene.cpp); this module reads the files and marshals."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from pathlib import Path

import numpy as np

from . import lib as _lib


@dataclass
class SceneBounds:
    bounds: np.ndarray        # (n, 2, 4) float32: (min.xyz, 0), (max.xyz, 0) — the ModelBounds buffer
    pipeline_keys: np.ndarray
    materials: np.ndarray
    centers: np.ndarray
    radii: np.ndarray
    scene_center: np.ndarray
    scene_radius: float

    @property
    def count(self) -> int:
        return self.bounds.shape[0]


def load_scene_bounds(scene_json_path, assets_root=None) -> SceneBounds:
    scene_json_path = Path(scene_json_path)
    assets_root = Path(assets_root) if assets_root is not None else scene_json_path.parent.parent  # RendererUtils.cpp:326-329
    L = _lib.load()
    text = scene_json_path.read_bytes()
    n = L.ur_scene_model_count(text)
    if n <= 0:
        raise ValueError(f"{scene_json_path}: no models")
    gltfs = []
    buf = C.create_string_buffer(1024)
    for i in range(n):
        if L.ur_scene_model_path(text, i, buf, 1024) < 0:
            raise ValueError(f"model {i} has no path")
        gltfs.append((assets_root / buf.value.decode()).read_bytes())
    arr = (C.c_char_p * n)(*gltfs)
    summary = _lib.SceneSummary()
    rc = L.ur_scene_extract(text, arr, n, None, 0, C.byref(summary))
    if rc != 0:
        raise ValueError(f"ur_scene_extract failed ({rc})")
    models = (_lib.SceneModel * summary.model_count)()
    rc = L.ur_scene_extract(text, arr, n, models, summary.model_count, C.byref(summary))
    if rc != 0:
        raise ValueError(f"ur_scene_extract failed ({rc})")
    m = summary.model_count
    bounds = np.zeros((m, 2, 4), np.float32)
    for i, x in enumerate(models):
        bounds[i, 0, :3] = x.bounds_min
        bounds[i, 1, :3] = x.bounds_max
    return SceneBounds(bounds, np.array([x.pipeline_key for x in models], np.uint32), np.array([x.material_index for x in models], np.uint32),
                       np.array([list(x.center) for x in models], np.float32), np.array([x.radius for x in models], np.float32),
                       np.array(list(summary.scene_center), np.float32), float(summary.scene_radius))


def _scene_texts(scene_json_path, assets_root):
    """(the scene JSON's bytes, the models' .gltf paths) of a scene file."""
    scene_json_path = Path(scene_json_path)
    assets_root = Path(assets_root) if assets_root is not None else scene_json_path.parent.parent  # RendererUtils.cpp:326-329
    L = _lib.load()
    text = scene_json_path.read_bytes()
    n = L.ur_scene_model_count(text)
    if n <= 0:
        raise ValueError(f"{scene_json_path}: no models")
    paths = []
    buf = C.create_string_buffer(1024)
    for i in range(n):
        if L.ur_scene_model_path(text, i, buf, 1024) < 0:
            raise ValueError(f"model {i} has no path")
        paths.append(assets_root / buf.value.decode())
    return text, paths


def plan_scene(scene_text: bytes, gltf_texts, mesh_base):
    """ur_scene_plan: (node records, draws) of a scene as structured arrays of lib.SceneNode and lib.ScenePlanDraw, the draws in
    ur_scene_extract's command order. mesh_base: per model, the number of meshes of the models in front."""
    L = _lib.load()
    n = len(gltf_texts)
    arr = (C.c_char_p * n)(*gltf_texts)
    base = (C.c_uint32 * n)(*[int(b) for b in mesh_base])
    node_count, draw_count = C.c_uint32(0), C.c_uint32(0)
    rc = L.ur_scene_plan(scene_text, arr, n, base, None, 0, C.byref(node_count), None, 0, C.byref(draw_count))
    if rc != 0:
        raise ValueError(f"ur_scene_plan failed ({rc})")
    nodes, draws = (_lib.SceneNode * node_count.value)(), (_lib.ScenePlanDraw * draw_count.value)()
    rc = L.ur_scene_plan(scene_text, arr, n, base, nodes, node_count.value, C.byref(node_count), draws, draw_count.value, C.byref(draw_count))
    if rc != 0:
        raise ValueError(f"ur_scene_plan failed ({rc})")
    return np.frombuffer(nodes, np.dtype(_lib.SceneNode)).copy(), np.frombuffer(draws, np.dtype(_lib.ScenePlanDraw)).copy()


def scene_draw_table(plan_draws, sections, material_base, material_counts) -> np.ndarray:
    """The lib.SceneDraw records of a plan: a draw's section (index_start, index_count) is sections[mesh][primitive] (Mesh.sections of the
    mesh among all models' meshes); its material record is material_base[model] + the glTF material index, or the model's default
    record (the last of its material_counts[model]) when the primitive names none or one out of range."""
    out = np.zeros(len(plan_draws), np.dtype(_lib.SceneDraw))
    for d, p in zip(out, plan_draws):
        model, material = int(p["model_index"]), int(p["material_index"])
        default = material_counts[model] - 1
        _, start, count = sections[int(p["mesh"])][int(p["primitive"])]
        d["node"], d["mesh"], d["constants_slot"], d["object_id"] = p["node"], p["mesh"], p["constants_slot"], p["object_id"]
        d["material"] = material_base[model] + (material if material < default else default)
        d["index_start"], d["index_count"] = start, count
    return out


def load_scene_tables(scene_json_path, assets_root=None, meshes=None, constants_stride: int = 608):
    """The four host tables of ur_scene_build composed from a scene file, and the mesh infos stacked on the device, as a
    hotpath.SceneTables ready for HotPath.build_scene. meshes: per model the hotpath.Mesh objects assets.load_gltf_meshes built from its
    file (device memory the commands will point into; kept alive by the result). The result also carries `plan` (the lib.ScenePlanDraw
    records: pipeline keys, glTF material indices, model indices, in command order) and `pipeline_keys`."""
    import json

    from . import assets, hotpath
    text, paths = _scene_texts(scene_json_path, assets_root)
    if meshes is None or len(meshes) != len(paths):
        raise ValueError(f"load_scene_tables: {len(paths)} models need their built meshes (assets.load_gltf_meshes per model)")
    gltf_texts = [p.read_bytes() for p in paths]
    mesh_base = np.concatenate([[0], np.cumsum([len(m) for m in meshes])]).astype(np.int64)
    nodes, plan = plan_scene(text, gltf_texts, mesh_base[:-1])
    factors = [assets.gltf_material_factors(json.loads(t)) for t in gltf_texts]
    material_counts = [len(f) for f in factors]
    material_base = np.concatenate([[0], np.cumsum(material_counts)])
    flat = [mesh for model in meshes for mesh in model]
    mesh_table = np.zeros(len(flat), np.dtype(_lib.SceneMesh))
    for record, mesh in zip(mesh_table, flat):
        record["vertices"], record["indices"] = mesh.vertices.data_ptr(), mesh.indices.data_ptr()
        record["vertex_bytes"], record["index_bytes"] = mesh.vertices.numel() * mesh.vertices.element_size(), mesh.indices.numel() * mesh.indices.element_size()
        record["stride"], record["index_format"] = 64, _lib.UR_RASTER_INDEX_FORMAT_R32_UINT
    draws = scene_draw_table(plan, [mesh.sections for mesh in flat], material_base, material_counts)
    tables = hotpath.SceneTables(nodes, mesh_table, hotpath.mesh_infos(flat), np.concatenate(factors), draws, slot_count=len(draws),
                                 constants_stride=constants_stride, keep=flat)
    tables.plan, tables.pipeline_keys = plan, plan["pipeline_key"].copy()
    return tables


def draw_offsets(keys) -> np.ndarray:
    """Draw-range offsets (ur_draw_ranges.offsets) over commands in command order: a new range starts wherever the key changes.
    uint32[R + 1] with offsets[0] = 0 and offsets[R] = len(keys). The reference's FIndirectDrawRanges break on every texture-handle
    change (DeferredRenderer.cpp:3327-3360), and the handle is per model: keys = arange(n), one range per command. Ranges per pipeline
    bucket: keys = SceneBounds.pipeline_keys. No commands: [0, 0], one empty range."""
    k = np.asarray(keys)
    if k.ndim != 1:
        raise ValueError("draw_offsets: keys must be one-dimensional")
    if k.size == 0:
        return np.zeros(2, np.uint32)
    starts = np.flatnonzero(k[1:] != k[:-1]) + 1
    return np.concatenate([[0], starts, [k.size]]).astype(np.uint32)
