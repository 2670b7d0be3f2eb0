"""The scene build without a GPU (include/ur_scene_build.h): hand-worked answers, ur_host_scene_build byte-equal to the
numpy restatement (tests/scene_build_ref.py) on seeded tables, the fixture scenes against ur_scene_extract, and planted errors that the
comparison must see. Everything is compared as bytes: no tolerance."""
import json

import numpy as np
import pytest

from tests import mesh_cases as M
from tests import scene_build_ref as R

F = np.float32
SIZES = (1, 63, 64, 65, 257, 4097)
ADDRESS = 0x7D0000000000


def frame():
    from unclerenderer_amd import lib
    return lib.SceneConstants.from_buffer_copy(R.frame_template())


def same_bytes(a, b):
    return all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in a)


def differing(a, b):
    return {k: int((a[k].view(np.uint8) != b[k].view(np.uint8)).sum()) for k in a if not np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8))}


def node(world=None, scale=(1, 1, 1), rotation=None, translate=(0, 0, 0)):
    n = np.zeros((), R.NODE)
    n["node_world"] = np.eye(4, dtype=F).reshape(-1) if world is None else np.asarray(world, F).reshape(-1)
    n["scale"], n["max_scale"] = scale, np.abs(np.asarray(scale, F)).max()
    n["rotation"] = np.eye(3, dtype=F).reshape(-1) if rotation is None else np.asarray(rotation, F).reshape(-1)
    n["translate"] = translate
    return n


def info(lo, hi, center=None, radius=None):
    i = np.zeros((), R.INFO)
    lo, hi = np.asarray(lo, F), np.asarray(hi, F)
    e = hi - lo
    i["min"], i["max"] = lo, hi
    i["center"] = F(0.5) * (lo + hi) if center is None else center
    i["radius"] = max(np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) * F(0.5), F(1)) if radius is None else radius
    return i


def both(nodes, infos, draws=None, slot_count=None):
    """The restatement's and the host build's outputs for small hand-made tables (one mesh record and one material per info); they must agree,
    and the restatement's are returned with the summary as a record."""
    from unclerenderer_amd import hostmath
    nodes, infos = np.atleast_1d(np.asarray(nodes)), np.atleast_1d(np.asarray(infos))
    if draws is None:
        draws = np.zeros(len(nodes), R.DRAW)
        draws["node"] = draws["mesh"] = draws["constants_slot"] = np.arange(len(nodes))
    slot_count = len(draws) if slot_count is None else slot_count
    meshes, materials = np.zeros(len(infos), R.MESH), np.zeros(1, R.FACTORS)
    want = R.build(nodes, meshes, infos, materials, draws, frame(), slot_count, 608, ADDRESS)
    got = hostmath.scene_build(nodes, meshes, infos, materials, draws, frame(), slot_count, 608, ADDRESS)
    assert same_bytes(want, got), differing(want, got)
    want["summary"] = np.frombuffer(want["summary"].tobytes(), R.SUMMARY)[0]
    return want


def test_identity_node_over_a_unit_box(urlib):
    out = both(node(), info((-1, -1, -1), (1, 1, 1)))
    r = np.sqrt(F(12)) * F(0.5)
    assert np.array_equal(out["bounds"][0], [[-1, -1, -1, 0], [1, 1, 1, 0]]) and np.array_equal(out["centers"][0], [0, 0, 0, r])
    assert np.array_equal(out["constants"][0, :64].view(F), np.eye(4, dtype=F).reshape(-1))
    s = out["summary"]
    e2 = (r + r) * (r + r)
    assert np.array_equal(s["scene_min"], [-r] * 3) and np.array_equal(s["scene_max"], [r] * 3) and np.array_equal(s["scene_center"], [0, 0, 0])
    assert s["scene_radius"] == np.sqrt((e2 + e2) + e2) * F(0.5) and (s["draw_count"], s["skipped_draws"]) == (1, 0)
    assert list(out["commands"][0, 8:16]) == [ADDRESS & 0xFFFFFFFF, ADDRESS >> 32, 0, 1, 0, 0, 0, 0]


def test_negative_scale_swaps_min_and_max(urlib):
    out = both(node(scale=(-2, 1, 1)), info((0, 0, 0), (1, 2, 3)))
    assert np.array_equal(out["bounds"][0], [[-2, 0, 0, 0], [0, 2, 3, 0]])  # x: max.x = 1 gives the minimum
    assert np.array_equal(out["centers"][0][:3], [-1, 1, 1.5]) and out["centers"][0][3] == (np.sqrt(F(14)) * F(0.5)) * F(2)  # radius x max |scale|


def test_quarter_turn_about_y(urlib):
    out = both(node(rotation=[[0, 0, -1], [0, 1, 0], [1, 0, 0]]), info((0, 0, 0), (1, 2, 3)))  # XMMatrixRotationRollPitchYaw(0, pi / 2, 0) with exact sines
    assert np.array_equal(out["bounds"][0], [[0, 0, -1, 0], [3, 2, 0, 0]])  # (x, y, z) -> (z, y, -x)
    assert np.array_equal(out["centers"][0][:3], [1.5, 1, -0.5])


def test_a_node_matrix_with_w_of_two_divides(urlib):
    world = np.eye(4, dtype=F)
    world[3, 3] = 2
    out = both(node(world), info((0, 0, 0), (1, 2, 3)))
    assert np.array_equal(out["bounds"][0], [[0, 0, 0, 0], [0.5, 1, 1.5, 0]]) and np.array_equal(out["centers"][0][:3], [0.25, 0.5, 0.75])
    assert out["constants"][0, :64].view(F)[15] == 2  # World itself is not divided


def test_w_of_zero(urlib):
    world = np.eye(4, dtype=F)
    world[3, 3] = 0
    out = both(node(world), info((0, 0, 0), (1, 2, 3)))
    # a coordinate of 0 gives 0 / 0, a NaN, which std::min and std::max pass over; a positive one gives +inf, which is not below FLT_MAX
    assert np.array_equal(out["bounds"][0], [[R.FLT_MAX] * 3 + [0], [np.inf] * 3 + [0]])
    assert np.array_equal(out["centers"][0][:3], [np.inf] * 3)
    assert np.array_equal(out["summary"]["scene_max"], [np.inf] * 3)


def test_a_nan_mesh_box(urlib):
    out = both(node(), info((np.nan, 0, 0), (1, 2, 3)))
    # the four corners with min.x are NaN in every coordinate (NaN * 0 is NaN); the other four give x = 1 alone and the whole y and z range
    assert np.array_equal(out["bounds"][0], [[1, 0, 0, 0], [1, 2, 3, 0]])
    assert np.isnan(out["centers"][0]).all()
    s = out["summary"]  # a NaN adds nothing to the box
    assert np.array_equal(s["scene_min"], [R.FLT_MAX] * 3) and np.array_equal(s["scene_max"], [-R.FLT_MAX] * 3) and np.array_equal(s["scene_center"], [0, 0, 0])
    assert s["scene_radius"] == np.inf and s["skipped_draws"] == 0


def test_centres_of_minus_and_plus_zero(urlib):
    """Centre +0 first, then centre -0 (0 / w with w = -1), both with radius 0: the serial std::min keeps the first, +0; the total order of the
    build takes -0. The one place where the summary differs from ur_scene_extract's fold, and only in the sign."""
    mirror = np.eye(4, dtype=F)
    mirror[3, 3] = -1
    out = both([node(), node(mirror)], [info((0, 0, 0), (0, 0, 0), radius=0), info((0, 0, 0), (0, 0, 0), radius=0)])
    assert np.array_equal(np.signbit(out["centers"][:, :3]), [[False] * 3, [True] * 3]) and np.array_equal(out["centers"][:, 3], [0, 0])
    s = out["summary"]
    assert np.array_equal(s["scene_min"], [0, 0, 0]) and np.signbit(s["scene_min"]).all()
    assert np.array_equal(s["scene_max"], [0, 0, 0]) and not np.signbit(s["scene_max"]).any()
    assert s["scene_radius"] == 1  # max(0, 1)


def test_all_draws_skipped(urlib):
    draws = np.zeros(4, R.DRAW)
    draws["node"], draws["mesh"], draws["material"], draws["constants_slot"] = [1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 1, 2, 4]
    out = both(node(), info((-1, -1, -1), (1, 1, 1)), draws, slot_count=4)
    assert not out["bounds"].view(np.uint8).any() and not out["commands"].any() and not out["centers"].view(np.uint8).any() and not out["constants"].any()
    s = out["summary"]
    assert np.array_equal(s["scene_min"], [R.FLT_MAX] * 3) and np.array_equal(s["scene_max"], [-R.FLT_MAX] * 3) and (s["draw_count"], s["skipped_draws"]) == (4, 4)


def prior(rng, D, slots, stride):
    """Outputs that hold something before the build: what it leaves alone must keep it."""
    return {"bounds": rng.integers(0, 256, (D, 2, 16), dtype=np.uint8).view(F).reshape(D, 2, 4), "commands": rng.integers(0, 1 << 32, (D, 16), dtype=np.uint64).astype(np.uint32),
            "constants": rng.integers(0, 256, (slots, stride), dtype=np.uint8), "centers": rng.integers(0, 256, (D, 16), dtype=np.uint8).view(F).reshape(D, 4),
            "summary": rng.integers(0, 256, 48, dtype=np.uint8)}


@pytest.mark.parametrize("stride", [608, 768])
@pytest.mark.parametrize("D", SIZES)
def test_host_build_is_byte_equal_to_the_restatement(urlib, D, stride):
    from unclerenderer_amd import hostmath
    nodes, meshes, infos, materials, draws, slots = R.seeded_tables(100 + D, D)
    init = prior(np.random.default_rng(D), D, slots, stride)
    want = R.build(nodes, meshes, infos, materials, draws, frame(), slots, stride, ADDRESS, out=init)
    got = hostmath.scene_build(nodes, meshes, infos, materials, draws, frame(), slots, stride, ADDRESS, out={k: v.copy() for k, v in init.items()})
    assert same_bytes(want, got), differing(want, got)
    assert np.array_equal(got["constants"][:, 608:], init["constants"][:, 608:])  # the gap up to the stride
    named = np.zeros(slots, bool)
    named[draws["constants_slot"][draws["constants_slot"] < slots]] = True
    assert np.array_equal(got["constants"][~named], init["constants"][~named])  # a slot no draw names
    # transforms only, after a node moved: bounds, centres, World and the summary are a full rebuild's; the rest keeps planted 0xA5
    nodes["translate"][0] += F(3)
    nodes["scale"][-1] *= F(-1.5)
    planted = {k: v.copy() for k, v in got.items()}
    planted["commands"][...] = 0xA5A5A5A5
    planted["constants"][:, 64:] = 0xA5
    full = R.build(nodes, meshes, infos, materials, draws, frame(), slots, stride, ADDRESS, out=got)
    moved = hostmath.scene_build(nodes, meshes, infos, materials, draws, frame(), slots, stride, ADDRESS, out=planted, transforms_only=True)
    assert same_bytes(moved, R.build(nodes, meshes, infos, materials, draws, frame(), slots, stride, ADDRESS, out=planted, transforms_only=True))
    for k in ("bounds", "centers", "summary"):
        assert np.array_equal(moved[k].view(np.uint8), full[k].view(np.uint8)), k
    assert np.array_equal(moved["constants"][:, :64], full["constants"][:, :64])
    assert (moved["commands"] == 0xA5A5A5A5).all() and (moved["constants"][:, 64:] == 0xA5).all()


@pytest.mark.parametrize("plant", R.PLANTS)
def test_planted_errors_fail(urlib, plant):
    """A wrong reading of the rule changes bytes of these tables, so the comparison above would fail for a build that made it."""
    from unclerenderer_amd import hostmath
    seen = {}
    for D in (65, 4097):
        nodes, meshes, infos, materials, draws, slots = R.seeded_tables(100 + D, D)
        got = hostmath.scene_build(nodes, meshes, infos, materials, draws, frame(), slots, 608, ADDRESS)
        wrong = R.build(nodes, meshes, infos, materials, draws, frame(), slots, 608, ADDRESS, plant=plant)
        assert not same_bytes(wrong, got), (plant, D)
        seen = differing(wrong, got)
    expected = {"product_order": "constants", "no_divide": "bounds", "corner_order": "bounds", "slot_is_command_index": "constants", "template_over_factors": "constants",
                "radius_without_node_scale": "centers"}[plant]
    assert expected in seen, (plant, seen)


SCENE_TWO_MODELS = {"models": [
    {"path": "BoxTextured/BoxTextured.gltf", "translate": [1.5, 0.25, -2.0], "rotate_euler": [10.0, 35.0, -20.0], "scale": [2.0, 0.5, -1.25]},
    {"path": "CompareNormal/CompareNormal.gltf", "translate": [-3.0, 0.0, 4.0], "rotate_euler": [0.0, 90.0, 0.0], "scale": [1.0, 1.0, 1.0]}]}


def scene_file(name, tmp_path):
    if name == "Duck":
        return M.ASSETS / "Scenes" / "Duck.json"
    path = tmp_path / "Scenes" / "two_models.json"
    path.parent.mkdir(exist_ok=True)
    path.write_text(json.dumps(SCENE_TWO_MODELS))
    return path


def host_scene(path):
    """The scene file's tables with the meshes built on the host, through the product's own composition (scene.plan_scene, scene.scene_draw_table,
    assets.gltf_material_factors), and ur_host_scene_build's outputs."""
    from unclerenderer_amd import assets, hostmath, lib, scene
    text, paths = scene._scene_texts(path, M.ASSETS)
    infos, sections, counts, factors = [], [], [], []
    for p in paths:
        gltf, data = assets.read_gltf(p)
        counts.append(len(gltf["meshes"]))
        factors.append(assets.gltf_material_factors(gltf))
        for m in range(len(gltf["meshes"])):
            _, _, s, i = hostmath.mesh_build(data, assets.gltf_mesh_primitives(gltf, m)[0])
            infos.append(bytes(i))
            sections.append(s)
    base = np.concatenate([[0], np.cumsum(counts)])
    nodes, plan = scene.plan_scene(text, [p.read_bytes() for p in paths], base[:-1])
    material_counts = [len(f) for f in factors]
    draws = scene.scene_draw_table(plan, sections, np.concatenate([[0], np.cumsum(material_counts)]), material_counts)
    meshes = np.zeros(len(infos), R.MESH)
    tables = (nodes, meshes, np.frombuffer(b"".join(infos), R.INFO), np.concatenate(factors), draws)
    return tables, plan, hostmath.scene_build(*tables, frame(), len(draws), 608, ADDRESS), sections


@pytest.mark.parametrize("name", ["Duck", "two_models"])
def test_fixture_scenes_match_ur_scene_extract(urlib, tmp_path, name):
    """Bounds, centres, radii, order and keys byte-equal to ur_scene_extract, which reads the accessors' min / max where the build reads the
    vertices: the three fixtures' vertex extrema are byte-equal to their accessor bounds (tests/mesh_ref.py). The summary is equal as values."""
    from unclerenderer_amd import scene
    path = scene_file(name, tmp_path)
    want = scene.load_scene_bounds(path, M.ASSETS)
    tables, plan, out, sections = host_scene(path)
    assert same_bytes(out, R.build(*tables, frame(), len(plan), 608, ADDRESS))
    assert len(plan) == want.count and np.array_equal(plan["pipeline_key"], want.pipeline_keys) and np.array_equal(plan["material_index"], want.materials)
    assert np.array_equal(out["bounds"].view(np.uint32), want.bounds.view(np.uint32))
    assert np.array_equal(out["centers"][:, :3].view(np.uint32), want.centers.view(np.uint32)) and np.array_equal(out["centers"][:, 3].view(np.uint32), want.radii.view(np.uint32))
    s = np.frombuffer(out["summary"].tobytes(), R.SUMMARY)[0]
    assert np.array_equal(s["scene_center"], want.scene_center) and s["scene_radius"] == F(want.scene_radius) and (s["draw_count"], s["skipped_draws"]) == (want.count, 0)
    # creation order: slots and ObjectIds are a permutation, ObjectId = slot + 1 (RendererUtils.cpp:306,485); the draws carry their sections
    assert sorted(plan["constants_slot"]) == list(range(len(plan))) and np.array_equal(plan["object_id"], plan["constants_slot"] + 1)
    draws = tables[4]
    for d, p in zip(draws, plan):
        assert (d["index_start"], d["index_count"]) == tuple(sections[p["mesh"]][p["primitive"]][1:])
    if name == "two_models":
        assert len(set(plan["model_index"])) == 2 and len(set(plan["mesh"])) >= 2 and len(set(draws["material"])) >= 2


def test_material_factors_follow_the_loader():
    from unclerenderer_amd import assets
    gltf = {"materials": [{"pbrMetallicRoughness": {"baseColorFactor": [0.5, 0.25, 0.125, 0.75], "metallicFactor": 0.0, "baseColorTexture": {
        "index": 0, "extensions": {"KHR_texture_transform": {"offset": [0.5, 0.25], "scale": [2, 4]}}}}, "emissiveFactor": [1, 2, 3], "alphaMode": "MASK"},
        {"alphaMode": "BLEND", "alphaCutoff": 0.9}], "textures": [{"source": 0}], "images": [{"uri": "x.png"}]}
    f = assets.gltf_material_factors(gltf)
    assert len(f) == 3 and f.dtype.itemsize == 176
    a, b, default = f
    assert list(a["BaseColor"]) == [0.5, 0.25, 0.125] and (a["BaseColorAlpha"], a["MetallicFactor"], a["RoughnessFactor"]) == (0.75, 0, 1)
    assert list(a["EmissiveFactor"]) == [1, 2, 3] and (a["AlphaMode"], a["AlphaCutoff"]) == (1, 0.5)
    assert list(a["transforms"][0]) == [0.5, 0.25, 2, 4] and list(a["transforms"][1]) == [1, 0, 0, 0] and list(a["transforms"][2]) == [0, 0, 1, 1]
    assert (b["AlphaMode"], b["AlphaCutoff"]) == (0, 0.5) and bytes(b) == bytes(default)  # the cutoff is read only under MASK
    del gltf["images"]  # the reference reads the materials only when textures and images are there
    assert all(bytes(r) == bytes(default) for r in assets.gltf_material_factors(gltf))
