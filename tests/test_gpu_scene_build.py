"""ur_scene_build on the GPU (include/ur_scene_build.h): every output byte-equal to the numpy restatement
(tests/scene_build_ref.py) on the seeded tables, whatever the scratch held; the transforms-only form after a node patch; and a closed loop:
a loaded Box and Duck through load_gltf_meshes, load_scene_tables and build_scene into the cull, the depth prepass and the GBuffer pass, byte-equal
to the same passes fed by pack_draw_commands, host-filled constants and ur_scene_extract's bounds."""
import json

import numpy as np
import pytest

from tests import mesh_cases as M
from tests import scene_build_ref as R
from tests.test_scene_build_ref import SIZES, differing, frame, same_bytes

pytestmark = pytest.mark.gpu


def device_tables(tables, slots, stride):
    from unclerenderer_amd.hotpath import SceneTables
    nodes, meshes, infos, materials, draws = tables
    return SceneTables(nodes, meshes, infos, materials, draws, slot_count=slots, constants_stride=stride)


def built_scene(D, slots, stride, fill, scratch_fill):
    """Outputs and scratch filled with a byte before the build."""
    import torch
    from unclerenderer_amd import lib
    from unclerenderer_amd.hotpath import BuiltScene
    need = int(lib.load().ur_scene_build_scratch_bytes(D))
    byte = lambda n, v: torch.full((n,), v, dtype=torch.uint8, device="cuda")  # noqa: E731
    return BuiltScene(byte(D * 32, fill).view(torch.float32).view(D, 2, 4), byte(D * 64, fill).view(torch.int32).view(D, 16), byte(slots * stride, fill).view(slots, stride),
                      byte(D * 16, fill).view(torch.float32).view(D, 4), byte(48, fill).view(torch.int32), byte(need, scratch_fill))


def host(built):
    import torch
    torch.cuda.synchronize()
    return {"bounds": built.bounds.cpu().numpy(), "commands": built.commands.cpu().numpy().view(np.uint32), "constants": built.constants.cpu().numpy(),
            "centers": built.centers.cpu().numpy(), "summary": built.summary.cpu().numpy().view(np.uint8)}


def filled(D, slots, stride, fill):
    return {"bounds": np.full((D, 2, 16), fill, np.uint8).view(np.float32).reshape(D, 2, 4), "commands": np.full((D, 64), fill, np.uint8).view(np.uint32).reshape(D, 16),
            "constants": np.full((slots, stride), fill, np.uint8), "centers": np.full((D, 16), fill, np.uint8).view(np.float32).reshape(D, 4), "summary": np.full(48, fill, np.uint8)}


@pytest.mark.parametrize("stride", [608, 768])
@pytest.mark.parametrize("D", SIZES)
def test_every_output_is_byte_equal_to_the_restatement(hotpath, D, stride):
    tables = R.seeded_tables(100 + D, D)
    slots = tables[-1]
    dev = device_tables(tables[:5], slots, stride)
    a = built_scene(D, slots, stride, 0x3C, 0xFF)
    hotpath.build_scene(dev, frame(), out=a)
    got = host(a)
    want = R.build(*tables[:5], frame(), slots, stride, a.constants.data_ptr(), out=filled(D, slots, stride, 0x3C))
    assert same_bytes(want, got), differing(want, got)
    assert (got["constants"][:, 608:] == 0x3C).all()
    # a second run, the scratch zeroed this time: the same bytes
    b = built_scene(D, slots, stride, 0x3C, 0x00)
    hotpath.build_scene(dev, frame(), out=b)
    again = host(b)
    want_b = R.build(*tables[:5], frame(), slots, stride, b.constants.data_ptr(), out=filled(D, slots, stride, 0x3C))
    assert same_bytes(want_b, again), differing(want_b, again)
    for k in ("bounds", "constants", "centers", "summary"):
        assert np.array_equal(got[k].view(np.uint8), again[k].view(np.uint8)), k


@pytest.mark.parametrize("D", [65, 4097])
def test_transforms_only_after_a_node_patch(hotpath, D):
    import torch
    nodes, meshes, infos, materials, draws, slots = R.seeded_tables(200 + D, D)
    dev = device_tables((nodes, meshes, infos, materials, draws), slots, 640)
    built = hotpath.build_scene(dev, frame())
    before = host(built)
    # the caller patches two nodes in the resident table and plants 0xA5 where the update must not write
    nodes["translate"][0] += np.float32(3)
    nodes["scale"][-1] *= np.float32(-1.5)
    nodes["max_scale"] = np.abs(nodes["scale"]).max(axis=1)
    dev.nodes.copy_(torch.from_numpy(nodes.view(np.uint8).reshape(-1).copy()).to("cuda"))
    built.commands.fill_(int(np.array([0xA5A5A5A5], np.uint32).view(np.int32)[0]))
    built.constants[:, 64:] = 0xA5
    hotpath.build_scene(dev, frame(), transforms_only=True, out=built)
    moved = host(built)
    full = R.build(nodes, meshes, infos, materials, draws, frame(), slots, 640, built.constants.data_ptr(), out=before)
    for k in ("bounds", "centers", "summary"):
        assert np.array_equal(moved[k].view(np.uint8), full[k].view(np.uint8)), k
    assert np.array_equal(moved["constants"][:, :64], full["constants"][:, :64])
    assert (moved["commands"] == 0xA5A5A5A5).all() and (moved["constants"][:, 64:] == 0xA5).all()
    assert not np.array_equal(moved["bounds"].view(np.uint8), before["bounds"].view(np.uint8))  # something did move
    # and a full rebuild in place restores the rest
    hotpath.build_scene(dev, frame(), out=built)
    rebuilt = host(built)
    want = R.build(nodes, meshes, infos, materials, draws, frame(), slots, 640, built.constants.data_ptr(), out=moved)
    assert same_bytes(want, rebuilt), differing(want, rebuilt)


def test_centers_may_be_null_and_the_summary_reads_back(hotpath):
    from unclerenderer_amd.hotpath import BuiltScene
    D = 257
    tables = R.seeded_tables(9, D)
    slots = tables[-1]
    a = built_scene(D, slots, 608, 0x11, 0xFF)
    b = BuiltScene(a.bounds, a.commands, a.constants, None, a.summary, a.scratch)
    out = hotpath.build_scene(device_tables(tables[:5], slots, 608), frame(), out=b)
    s = out.scene_summary()
    want = R.build(*tables[:5], frame(), slots, 608, a.constants.data_ptr(), out=filled(D, slots, 608, 0x11))
    assert bytes(s) == want["summary"].tobytes() and (s.draw_count, s.skipped_draws) == (D, 4)
    got = host(a)
    assert (got["centers"].view(np.uint8) == 0x11).all()
    for k in ("bounds", "commands", "constants"):
        assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), k


BOX_SCENE = {"models": [{"path": "BoxTextured/BoxTextured.gltf", "translate": [0.25, -0.5, 1.0], "rotate_euler": [20.0, 35.0, -10.0], "scale": [1.5, 0.75, -1.25]}]}


@pytest.mark.parametrize("name", ["Box", "Duck"])
def test_closed_loop_into_the_cull_and_the_raster_passes(hotpath, tmp_path, name):
    import torch
    from tests import gbuffer_gpu as GG
    from unclerenderer_amd import assets, hostmath, lib, scene
    from unclerenderer_amd.hotpath import pack_draw_commands, to_device
    if name == "Duck":
        path = M.ASSETS / "Scenes" / "Duck.json"
    else:
        path = tmp_path / "Scenes" / "box.json"
        path.parent.mkdir()
        path.write_text(json.dumps(BOX_SCENE))
    _, model_paths = scene._scene_texts(path, M.ASSETS)
    meshes = [assets.load_gltf_meshes(p, hotpath) for p in model_paths]
    tables = scene.load_scene_tables(path, M.ASSETS, meshes)
    template = frame()
    built = hotpath.build_scene(tables, template)
    s = built.scene_summary()
    n = tables.draw_count
    assert (s.draw_count, s.skipped_draws) == (n, 0)

    # the camera looks at the scene's centre from outside its sphere
    eye = (s.scene_center[0], s.scene_center[1], s.scene_center[2] - 2.5 * s.scene_radius)
    view, proj = hostmath.look_to_lh(eye, (0.0, 0.0, 1.0)), hostmath.reverse_z_projection(1.0, 1.0, 0.1)
    w = h = 64
    culling = hostmath.pack_culling_constants(view, proj, n, False, 0, 0, 0)

    def passes(bounds, commands):
        commands = commands.clone()
        stats = torch.zeros(2, dtype=torch.int32, device="cuda")
        hotpath.cull_indirect_args(culling, bounds, None, None, commands, stats)
        depth = torch.full((h, w), float("nan"), dtype=torch.float32, device="cuda")
        depth_stats = torch.zeros(6, dtype=torch.int32, device="cuda")
        hotpath.depth_prepass(view, proj, commands, depth, stats=depth_stats)

        class Draws:
            pass
        dd = Draws()
        dd.commands = commands
        out = GG.run(hotpath, dd, view, proj, depth, w, h, object_id=True)
        out["depth"], out["depth_stats"], out["cull_stats"] = depth.cpu().numpy(), depth_stats.cpu().numpy().view(np.uint32), stats.cpu().numpy().view(np.uint32)
        out["commands"] = commands.cpu().numpy().view(np.uint32).reshape(n, 16)
        return out

    got = passes(built.bounds, built.commands)

    # the host's way: ur_scene_extract's bounds, constants filled field by field, pack_draw_commands
    extracted = scene.load_scene_bounds(path, M.ASSETS)
    flat = [m for model in meshes for m in model]
    nodes, draws = tables.nodes.cpu().numpy().view(R.NODE), tables.draws.cpu().numpy().view(R.DRAW)
    materials = tables.materials.cpu().numpy().view(R.FACTORS)
    infos = tables.mesh_infos.cpu().numpy().view(np.uint8).reshape(-1).view(R.INFO)
    world = R.place(nodes[draws["node"]], infos[draws["mesh"]])[0]
    records = np.repeat(np.frombuffer(bytes(template), R.CONSTANTS, 1), n)
    for k, d in enumerate(draws):
        m = materials[d["material"]]
        records[k]["World"] = world[k].reshape(-1)
        for field in ("BaseColor", "EmissiveFactor", "MetallicFactor", "RoughnessFactor", "BaseColorAlpha", "AlphaCutoff", "AlphaMode", "transforms"):
            records[k][field] = m[field]
        records[k]["ObjectId"] = d["object_id"]
    host_constants = to_device(records.view(np.uint8).reshape(n, 608))
    dicts = [{"vertices": flat[d["mesh"]].vertices, "stride": 64, "indices": flat[d["mesh"]].indices, "constants": host_constants, "constants_offset": 608 * k,
              "start_index": int(d["index_start"]), "index_count": int(d["index_count"]), "base_vertex": 0} for k, d in enumerate(draws)]
    want = passes(to_device(extracted.bounds), to_device(pack_draw_commands(dicts)))

    assert got["depth_stats"][1] == 0 and got["stats"][1] == 0, (got["depth_stats"], got["stats"])  # nothing unsupported
    assert (got["depth"] > 0).sum() > 50, "the model covers some texels"
    assert set(np.unique(got["object_id"])) - {0, 0x5A5A5A5A} <= set(int(i) for i in draws["object_id"]) and (got["object_id"] == draws["object_id"][0]).any()
    for key in ("cull_stats", "depth", "depth_stats", "keys", "A", "B", "C", "hdr", "object_id", "stats"):
        assert np.array_equal(got[key].view(np.uint8), want[key].view(np.uint8)), key
    # the commands are pack_draw_commands' but for the constants' address and word 14, the slot
    mask = np.ones(16, bool)
    mask[[8, 9, 14]] = False
    assert np.array_equal(got["commands"][:, mask], want["commands"][:, mask]) and np.array_equal(got["commands"][:, 14], draws["constants_slot"])
    assert (got["commands"][:, 11] == 1).all()  # the cull kept every draw in view
    # and the device's bounds are ur_scene_extract's
    assert np.array_equal(built.bounds.cpu().numpy().view(np.uint32), extracted.bounds.view(np.uint32))
