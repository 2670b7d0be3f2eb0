"""ur_mesh_build on the GPU: for every case of tests/mesh_cases.py - the hand cases, the three fixtures, the seeded
soups, the long segments, the index widths, modes and strides, the vertex counts at the scan's edges - the vertices, the indices and the
info record are byte-equal to the numpy restatement (tests/mesh_ref.py), with the scratch arriving full of 0xFF; two runs are
byte-equal; and a loaded Box and Duck go through mesh_draws into ur_depth_prepass and ur_gbuffer_pass and give the bytes of the same calls
over the restatement's buffers."""
import numpy as np
import pytest

from tests import mesh_cases as M
from tests import mesh_ref as R

pytestmark = pytest.mark.gpu


def _build(hotpath, name, fill=0xFF):
    import torch
    from unclerenderer_amd import hostmath
    data, prims = M.case(name)
    records = M.host_primitives(prims)
    layout, _ = hostmath.mesh_layout(records, len(data))
    scratch = torch.full((int(layout.scratch_bytes),), fill, dtype=torch.uint8, device="cuda")
    mesh = hotpath.build_mesh(data, records, scratch=scratch)
    torch.cuda.synchronize()
    return mesh.vertices.cpu().numpy().view(np.uint32), mesh.indices.cpu().numpy().view(np.uint32), mesh.sections, mesh.info.cpu().numpy().tobytes()


def _same(got, name):
    vertices, indices, sections, info = M.expected(name)
    gv, gi, gs, ginfo = got
    assert np.array_equal(gi, indices), (name, "indices", np.flatnonzero(gi != indices)[:8])
    assert gs == sections, (name, gs, sections)
    rows = np.flatnonzero((gv != vertices).any(1))
    assert rows.size == 0, (name, f"{rows.size} vertices differ, first {rows[:8]}", gv[rows[0]].view(np.float32), vertices[rows[0]].view(np.float32))
    assert ginfo == R.info_bytes(info), (name, np.frombuffer(ginfo, np.uint32), np.frombuffer(R.info_bytes(info), np.uint32))


@pytest.mark.parametrize("name", M.names())
def test_bytes_equal_the_restatement(hotpath, name):
    _same(_build(hotpath, name), name)


def test_the_long_cases_take_the_queue():
    """What the cases are for: a segment above one workgroup's 2048-corner LDS tile, two queued vertices, and the lane path's bound."""
    _, indices, _, info = M.expected("fans")
    valence = np.bincount(indices)
    assert info["normals_regenerated"] == info["tangents_regenerated"] == 1
    assert valence.max() == 5000 and (valence > M.LANE_SEGMENT).sum() == 2 and sorted(valence)[-2] == 300
    assert np.bincount(M.expected("valence_at_bound")[1]).max() == M.LANE_SEGMENT
    assert np.bincount(M.expected("valence_above_bound")[1]).max() == M.LANE_SEGMENT + 1
    soup = M.expected("soup")[3]
    assert soup["normals_regenerated"] == soup["tangents_regenerated"] == 1 and soup["out_of_range_triangles"] == 3 and soup["skipped_determinant_triangles"] > 10


@pytest.mark.parametrize("name", ["soup", "fans"])
def test_two_runs_are_byte_equal_whatever_the_scratch_held(hotpath, name):
    a, b = _build(hotpath, name, 0xFF), _build(hotpath, name, 0x00)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[3] == b[3]
    _same(b, name)


@pytest.mark.parametrize("name", ["Box", "Duck"])
def test_a_loaded_model_goes_straight_into_the_passes(hotpath, name):
    import torch
    from unclerenderer_amd import assets, hostmath
    from unclerenderer_amd.hotpath import mesh_draws, pack_draw_commands, to_device
    from tests import gbuffer_gpu as GG
    from tests import gbuffer_ref as G
    folder = {"Box": "BoxTextured/BoxTextured.gltf", "Duck": "Duck/Duck.gltf"}[name]
    meshes = assets.load_gltf_meshes(M.ASSETS / folder, hotpath)
    assert len(meshes) == 1 and meshes[0].materials == [0]
    mesh = meshes[0]
    vertices, indices, sections, info = M.expected(f"{name}_0")
    # the model in front of a camera at the origin looking down +z
    scale = np.float32(1.0 / max(float(info["radius"]), 1e-3))
    world = np.diag([scale, scale, scale, 1.0]).astype(np.float32)
    world[3, :3] = -info["center"] * scale + np.array([0, 0, 2.5], np.float32)
    constants = G.GDraw(vertices.view(np.uint8).reshape(-1), indices, world).constants()
    view = hostmath.look_to_lh((0.0, 0.0, 0.0), (0.0, 0.0, 1.0))
    proj = hostmath.reverse_z_projection(1.0, 1.0, 0.1)
    w = h = 64

    def passes(commands):
        depth = torch.full((h, w), float("nan"), dtype=torch.float32, device="cuda")
        stats = torch.zeros(6, dtype=torch.int32, device="cuda")
        hotpath.depth_prepass(view, proj, commands, depth, stats=stats)

        class Draws:
            pass
        dd = Draws()
        dd.commands = commands
        out = GG.run(hotpath, dd, view, proj, depth, w, h)
        out["depth"], out["depth_stats"] = depth.cpu().numpy(), stats.cpu().numpy().view(np.uint32)
        return out

    c = to_device(constants)
    got = passes(to_device(pack_draw_commands(mesh_draws(mesh, c))))
    ref_mesh = type(mesh)(to_device(np.array(vertices)), to_device(np.array(indices)), sections, None)
    want = passes(to_device(pack_draw_commands(mesh_draws(ref_mesh, c))))
    assert got["depth_stats"][1] == 0 and got["stats"][1] == 0, (got["depth_stats"], got["stats"])  # nothing unsupported
    assert (got["depth"] > 0).sum() > 100, "the model covers some texels"
    for key in ("depth", "depth_stats", "keys", "A", "B", "C", "hdr", "object_id", "stats"):
        assert np.array_equal(got[key].view(np.uint8), want[key].view(np.uint8)), key
