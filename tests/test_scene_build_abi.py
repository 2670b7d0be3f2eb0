"""The scene build's ABI without a GPU (include/ur_scene_build.h): struct layouts against a compiled probe, the symbols declared,
exported and bound, csrc/scene_host.cpp built by the plain host compiler (and run under ASan / UBSan by a stand-alone program), every refusal
of ur_scene_build with its text - decided before a device is needed - the Python routing and the kernels' resources from the built library's
metadata."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

from tests import scene_build_ref as R
from tests.test_bcn_abi import ROOT, _cxx

CSRC = ROOT / "unclerenderer_amd" / "csrc"
NEW = {"ur_scene_build_scratch_bytes": "ur_scene_build.h", "ur_scene_build": "ur_scene_build.h", "ur_host_scene_build": "ur_host.h", "ur_scene_plan": "ur_scene.h"}


def test_struct_layouts_against_a_compiled_probe(tmp_path):
    from unclerenderer_amd import lib
    src = tmp_path / "probe.cpp"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ur_scene_build.h"\n#include "ur_scene.h"\n#include "ur_host.h"\n'
                   'int main() { printf("%zu %zu %zu %zu %zu %zu %zu %zu  %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu  %u %u %u\\n", sizeof(ur_scene_node), sizeof(ur_scene_mesh), '
                   'sizeof(ur_scene_material_factors), sizeof(ur_scene_draw), sizeof(ur_scene_build_summary), sizeof(ur_scene_build_tables), sizeof(ur_scene_build_outputs), '
                   'sizeof(ur_scene_plan_draw), offsetof(ur_scene_node, scale), offsetof(ur_scene_node, max_scale), offsetof(ur_scene_node, rotation), '
                   'offsetof(ur_scene_node, translate), offsetof(ur_scene_node, reserved), offsetof(ur_scene_mesh, vertex_bytes), offsetof(ur_scene_material_factors, AlphaMode), '
                   'offsetof(ur_scene_material_factors, transforms), offsetof(ur_scene_build_summary, draw_count), offsetof(ur_scene_build_outputs, constants_stride), '
                   'UR_SCENE_BUILD_MAX_STREAM_OPS, UR_SCENE_BUILD_TRANSFORMS_ONLY, UR_SCENE_BUILD_MAX_DRAWS); return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.run([_cxx(), "-std=c++17", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [144, 32, 176, 32, 48, 56, 48, 32, 64, 76, 80, 116, 128, 16, 40, 48, 40, 40, 3, 1, 1 << 24]
    N, F, S, O = lib.SceneNode, lib.SceneMaterialFactors, lib.SceneBuildSummary, lib.SceneBuildOutputs
    assert [C.sizeof(N), C.sizeof(lib.SceneMesh), C.sizeof(F), C.sizeof(lib.SceneDraw), C.sizeof(S), C.sizeof(lib.SceneBuildTables), C.sizeof(O), C.sizeof(lib.ScenePlanDraw),
            N.scale.offset, N.max_scale.offset, N.rotation.offset, N.translate.offset, N.reserved.offset, lib.SceneMesh.vertex_bytes.offset, F.AlphaMode.offset,
            F.transforms.offset, S.draw_count.offset, O.constants_stride.offset, lib.UR_SCENE_BUILD_MAX_STREAM_OPS, lib.UR_SCENE_BUILD_TRANSFORMS_ONLY,
            lib.UR_SCENE_BUILD_MAX_DRAWS] == got
    # the restatement's records and the product's are the same layouts
    for mine, theirs in ((R.NODE, N), (R.MESH, lib.SceneMesh), (R.FACTORS, F), (R.DRAW, lib.SceneDraw), (R.SUMMARY, S), (R.INFO, lib.MeshInfo), (R.CONSTANTS, lib.SceneConstants)):
        other = np.dtype(theirs)
        assert mine.itemsize == other.itemsize and [mine.fields[n][1] for n in mine.names if n in other.names] == [other.fields[n][1] for n in mine.names if n in other.names]


def test_symbols_declared_exported_and_bound(urlib):
    from unclerenderer_amd import assets, hostmath, hotpath, lib, scene
    strip = lambda text: re.sub(r"/\*.*?\*/", "", text, flags=re.S)  # noqa: E731
    for name, header in NEW.items():
        assert re.search(r"\b%s\s*\(" % name, strip((ROOT / "include" / header).read_text())), name
        assert name in lib.SIGNATURES and getattr(urlib, name) is not None
    assert callable(hotpath.HotPath.build_scene) and callable(hotpath.mesh_infos) and callable(hostmath.scene_build)
    assert callable(assets.gltf_material_factors) and callable(scene.load_scene_tables) and callable(scene.plan_scene)
    assert "scene_build" not in strip((ROOT / "include" / "ur_frame.h").read_text())  # nothing is wired into the frame
    assert urlib.ur_scene_build_scratch_bytes(0) == 0 and urlib.ur_scene_build_scratch_bytes(1 << 24) == 0
    for D in (1, 64, 65, (1 << 24) - 1):
        need = urlib.ur_scene_build_scratch_bytes(D)
        assert need % 16 == 0 and need == 32 * ((D + 63) // 64)


def test_the_host_unit_builds_with_the_plain_compiler_and_builds_the_same(tmp_path, urlib):
    so = tmp_path / "libscene_host.so"
    subprocess.run([_cxx(), "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", str(CSRC / "scene_host.cpp"), "-o", str(so)], check=True)
    from unclerenderer_amd import hostmath, lib
    frame = lib.SceneConstants.from_buffer_copy(R.frame_template())
    nodes, meshes, infos, materials, draws, slots = R.seeded_tables(11, 257)
    plain = hostmath.scene_build(nodes, meshes, infos, materials, draws, frame, slots, 624, 1 << 40, library=C.CDLL(str(so)))
    ours = hostmath.scene_build(nodes, meshes, infos, materials, draws, frame, slots, 624, 1 << 40)
    want = R.build(nodes, meshes, infos, materials, draws, frame, slots, 624, 1 << 40)
    assert all(np.array_equal(plain[k].view(np.uint8), want[k].view(np.uint8)) and np.array_equal(ours[k].view(np.uint8), want[k].view(np.uint8)) for k in want)


SANITIZE_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "ur_host.h"
// argv[1]: a file of { u32 nodes, meshes, materials, draws, slots, stride, flags, pad; the five tables }. Every table and every output is a
// heap buffer of exactly its size, so that a read or write past one is seen.
static void* take(FILE* f, size_t bytes)
{
    void* p = malloc(bytes ? bytes : 1);
    if (bytes && fread(p, 1, bytes, f) != bytes) exit(2);
    return p;
}
int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    unsigned h[8];
    if (fread(h, 4, 8, f) != 8) return 2;
    ur_scene_build_tables t;
    t.node_count = h[0]; t.mesh_count = h[1]; t.material_count = h[2]; t.draw_count = h[3];
    t.nodes = (const ur_scene_node*)take(f, sizeof(ur_scene_node) * (size_t)h[0]);
    t.meshes = (const ur_scene_mesh*)take(f, sizeof(ur_scene_mesh) * (size_t)h[1]);
    t.mesh_infos = (const ur_mesh_info*)take(f, sizeof(ur_mesh_info) * (size_t)h[1]);
    t.materials = (const ur_scene_material_factors*)take(f, sizeof(ur_scene_material_factors) * (size_t)h[2]);
    t.draws = (const ur_scene_draw*)take(f, sizeof(ur_scene_draw) * (size_t)h[3]);
    ur_scene_constants* frame = (ur_scene_constants*)take(f, sizeof(ur_scene_constants));
    fclose(f);
    const size_t D = h[3], constants = (size_t)h[4] * h[5];
    ur_scene_build_outputs o;
    o.bounds = (ur_float4*)calloc(2 * D, sizeof(ur_float4));
    o.commands = calloc(D, 64);
    o.constants = calloc(constants, 1);
    o.centers = (ur_float4*)calloc(D, sizeof(ur_float4));
    o.summary = (ur_scene_build_summary*)calloc(1, sizeof(ur_scene_build_summary));
    o.slot_count = h[4]; o.constants_stride = h[5];
    int rc = ur_host_scene_build(&t, frame, &o, 0x100000ull, 0);
    if (rc == 0 && h[6]) rc = ur_host_scene_build(&t, frame, &o, 0x100000ull, h[6]);
    unsigned long long sum = 0;
    const unsigned char* parts[5] = {(unsigned char*)o.bounds, (unsigned char*)o.commands, (unsigned char*)o.constants, (unsigned char*)o.centers, (unsigned char*)o.summary};
    const size_t sizes[5] = {32 * D, 64 * D, constants, 16 * D, sizeof(ur_scene_build_summary)};
    for (int k = 0; k < 5; ++k)
        for (size_t i = 0; i < sizes[k]; ++i) sum += parts[k][i];
    printf("%d %llu %u\n", rc, sum, o.summary->skipped_draws);
    free((void*)t.nodes); free((void*)t.meshes); free((void*)t.mesh_infos); free((void*)t.materials); free((void*)t.draws); free(frame);
    free(o.bounds); free(o.commands); free(o.constants); free(o.centers); free(o.summary);
    return rc == 0 ? 0 : 1;
}
"""


@pytest.mark.parametrize("D,stride,flags", [(1, 608, 0), (65, 768, 0), (257, 608, 1)])
def test_host_build_under_asan_and_ubsan(tmp_path, D, stride, flags):
    """A stand-alone program with its own main, csrc/scene_host.cpp compiled in with -fsanitize=address,undefined: no Python, no device."""
    main = tmp_path / "scene_sanitize_main.cpp"
    main.write_text(SANITIZE_MAIN)
    exe = tmp_path / "scene_sanitize"
    subprocess.run([_cxx(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", f"-I{ROOT / 'include'}", str(main),
                    str(CSRC / "scene_host.cpp"), "-o", str(exe)], check=True)
    nodes, meshes, infos, materials, draws, slots = R.seeded_tables(3 * D, D)
    blob = tmp_path / "scene.bin"
    blob.write_bytes(np.uint32([len(nodes), len(meshes), len(materials), D, slots, stride, flags, 0]).tobytes() + nodes.tobytes() + meshes.tobytes() + infos.tobytes()
                     + materials.tobytes() + draws.tobytes() + R.frame_template())
    r = subprocess.run([str(exe), str(blob)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    want = R.build(nodes, meshes, infos, materials, draws, R.frame_template(), slots, stride, 0x100000)
    total = sum(int(want[k].view(np.uint8).sum(dtype=np.uint64)) for k in want)
    skipped = int(np.frombuffer(want["summary"].tobytes(), R.SUMMARY)[0]["skipped_draws"])
    assert r.stdout.split() == ["0", str(total), str(skipped)]


def test_build_refusals_that_need_no_device(urlib):
    """Every check comes before the context is looked at: a stand-in context is enough, the addresses are numbers and none is dereferenced."""
    from unclerenderer_amd import lib
    stand_in = C.create_string_buffer(4096)
    frame = lib.SceneConstants()
    D = 100
    need = int(urlib.ur_scene_build_scratch_bytes(D))
    base = dict(ctx=C.addressof(stand_in), frame=C.byref(frame), scratch=0xA00000, scratch_bytes=need, flags=0,
                nodes=0x100000, meshes=0x200000, mesh_infos=0x300000, materials=0x400000, draws=0x500000, node_count=7, mesh_count=3, material_count=2, draw_count=D,
                bounds=0x600000, commands=0x700000, constants=0x800000, centers=0x900000, summary=0x980000, constants_stride=608, slot_count=D)

    def call(**kw):
        a = dict(base, **kw)
        t = lib.SceneBuildTables(a["nodes"], a["meshes"], a["mesh_infos"], a["materials"], a["draws"], a["node_count"], a["mesh_count"], a["material_count"], a["draw_count"])
        o = lib.SceneBuildOutputs(a["bounds"], a["commands"], a["constants"], a["centers"], a["summary"], a["constants_stride"], a["slot_count"])
        tables = C.byref(t) if a.get("tables", True) else None
        outputs = C.byref(o) if a.get("outputs", True) else None
        return urlib.ur_scene_build(a["ctx"], tables, a["frame"], outputs, a["scratch"], a["scratch_bytes"], a["flags"])

    def refused(text, **kw):
        rc = call(**kw)
        assert rc == lib.UR_EINVAL and text in urlib.ur_last_error().decode(), (text, kw, rc, urlib.ur_last_error())

    refused("null context or scratch", ctx=None)
    refused("null context or scratch", scratch=None)
    refused("null tables, frame or outputs", tables=False)
    refused("null tables, frame or outputs", frame=None)
    refused("null tables, frame or outputs", outputs=False)
    for name in ("nodes", "meshes", "mesh_infos", "materials", "draws"):
        refused("null table", **{name: None})
        refused(f"{name} not 16-byte aligned", **{name: base[name] + 8})
    for name in ("bounds", "commands", "constants", "summary"):
        refused("null bounds, commands, constants or summary", **{name: None})
        refused(f"{name} not 16-byte aligned", **{name: base[name] + 4})
    refused("centers not 16-byte aligned", centers=base["centers"] + 8)
    refused("scratch not 16-byte aligned", scratch=base["scratch"] + 8)
    refused("0 draws", draw_count=0)
    refused("16777216 draws", draw_count=1 << 24)
    for name in ("node_count", "mesh_count", "material_count"):
        refused("an empty table", **{name: 0})
    refused("no constants slots", slot_count=0)
    refused("constants stride 592", constants_stride=592)
    refused("constants stride 616", constants_stride=616)
    refused("unknown flag bits 0x2", flags=3)
    refused("scratch bytes", scratch_bytes=need - 1)
    refused("bounds and commands overlap", commands=base["bounds"] + 32 * D - 16)
    refused("bounds and constants overlap", constants=base["bounds"] - 608 * D + 16)
    refused("commands and centers overlap", centers=base["commands"] + 64)
    refused("constants and summary overlap", summary=base["constants"] + 608 * D - 16)
    refused("constants and summary overlap", summary=base["constants"] + 768 * D - 16, constants_stride=768)
    refused("centers and summary overlap", summary=base["centers"] + 16 * D - 16)
    refused("bounds and scratch overlap", scratch=base["bounds"] + 16)
    refused("summary and scratch overlap", scratch=base["summary"] + 32)
    refused("bounds and nodes overlap", nodes=base["bounds"] + 16)
    refused("commands and meshes overlap", meshes=base["commands"] - 32 * 3 + 16)
    refused("constants and mesh_infos overlap", mesh_infos=base["constants"] + 160)
    refused("centers and materials overlap", materials=base["centers"] + 16 * D - 16)
    refused("summary and draws overlap", draws=base["summary"] - 32 * D + 16)
    refused("scratch and draws overlap", draws=base["scratch"] + 16)
    # the tables are only read and may share bytes; centers may be null: these pass every check (and would go on to launch, so they are not called)
    # the host twin refuses what it can decide
    o = lib.SceneBuildOutputs(0, 0, 0, 0, 0, 608, 1)
    assert urlib.ur_host_scene_build(None, C.byref(frame), C.byref(o), 0, 0) == lib.UR_EINVAL
    t = lib.SceneBuildTables(1, 1, 1, 1, 1, 1, 1, 1, 1)
    assert urlib.ur_host_scene_build(C.byref(t), C.byref(frame), C.byref(o), 0, 0) == lib.UR_EINVAL  # null outputs
    assert urlib.ur_host_scene_build(C.byref(t), C.byref(frame), C.byref(lib.SceneBuildOutputs(1, 1, 1, 0, 1, 600, 1)), 0, 0) == lib.UR_EINVAL
    assert urlib.ur_host_scene_build(C.byref(t), C.byref(frame), C.byref(lib.SceneBuildOutputs(1, 1, 1, 0, 1, 608, 1)), 0, 2) == lib.UR_EINVAL
    n = C.c_uint32(0)
    assert urlib.ur_scene_plan(b"{}", None, 0, None, None, 0, C.byref(n), None, 0, C.byref(n)) == -1


def test_python_routing(urlib, monkeypatch):
    from unclerenderer_amd import hostmath, hotpath, lib

    class T:  # a stand-in for a device tensor: an address and a size
        is_cuda = True

        def __init__(self, address, nbytes):
            self.address, self.nbytes = address, nbytes

        def is_contiguous(self):
            return True

        def data_ptr(self):
            return self.address

        def numel(self):
            return self.nbytes

        def element_size(self):
            return 1

    monkeypatch.setattr(hotpath.torch, "Tensor", T)
    tables = hotpath.SceneTables(T(0x1000, 144 * 3), T(0x2000, 32 * 2), T(0x3000, 56 * 2), T(0x4000, 176 * 5), T(0x5000, 32 * 9), slot_count=12, constants_stride=768)
    assert (tables.node_count, tables.mesh_count, tables.material_count, tables.draw_count, tables.slot_count) == (3, 2, 5, 9, 12)
    record = tables.record()
    assert (record.nodes, record.draws, record.draw_count) == (0x1000, 0x5000, 9)
    with pytest.raises(ValueError, match="info records"):
        hotpath.SceneTables(T(0x1000, 144), T(0x2000, 64), T(0x3000, 56), T(0x4000, 176), T(0x5000, 32))

    class NoDevice(hotpath.HotPath):
        def __init__(self):
            self._L, self._ctx = urlib, None
    with pytest.raises(ValueError, match="transforms_only"):
        NoDevice().build_scene(tables, lib.SceneConstants(), transforms_only=True)
    out = hotpath.BuiltScene(T(0x6000, 32 * 9), T(0x7000, 64 * 9), T(0x8000, 768 * 12), None, T(0x9000, 48), T(0xA000, 32))
    with pytest.raises(lib.UrError, match="null context"):  # the call reaches the library with the records filled in
        NoDevice().build_scene(tables, lib.SceneConstants(), out=out)
    with pytest.raises(ValueError, match="info records"):
        hostmath.scene_build(np.zeros(144, np.uint8), np.zeros(64, np.uint8), np.zeros(56, np.uint8), np.zeros(176, np.uint8), np.zeros(32, np.uint8), lib.SceneConstants(), 1)
    with pytest.raises(ValueError, match="ur_host_scene_build failed"):
        hostmath.scene_build(np.zeros(144, np.uint8), np.zeros(32, np.uint8), np.zeros(56, np.uint8), np.zeros(176, np.uint8), np.zeros(32, np.uint8), lib.SceneConstants(), 1, 600)


def test_scene_kernels_use_no_scratch_and_spill_nothing(urlib, tmp_path):
    from tests.code_objects import library_kernels
    kernels = {k: v for k, v in library_kernels(tmp_path).items() if re.search(r"scene_\w+_kernel", k)}
    assert len(kernels) == 3, sorted(kernels)  # the build in its two forms and the finish
    for name, meta in kernels.items():
        assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0 and meta["sgpr_spill_count"] == 0, (name, meta)
        assert meta["vgpr_count"] <= 128, (name, meta)
        print(name, meta["vgpr_count"], meta["sgpr_count"])
