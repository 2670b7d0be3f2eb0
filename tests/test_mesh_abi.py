"""The mesh build's ABI without a GPU (include/ur_mesh.h): struct layouts against a compiled probe, the symbols
declared, exported and bound, csrc/mesh_host.cpp built by the plain host compiler (and run under ASan / UBSan by a stand-alone program),
every refusal of ur_mesh_layout_of and ur_mesh_build with its text - decided before a device is needed - the layout's sums, the
Python routing and the new kernels' resources from the built library's metadata."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

from tests import mesh_cases as M
from tests import mesh_ref as R
from tests.test_bcn_abi import ROOT, _cxx

CSRC = ROOT / "unclerenderer_amd" / "csrc"
NEW = {"ur_mesh_layout_of": "ur_mesh.h", "ur_mesh_build": "ur_mesh.h", "ur_host_mesh_build": "ur_host.h"}


def test_struct_layouts_against_a_compiled_probe(tmp_path):
    from unclerenderer_amd import lib
    src = tmp_path / "probe.cpp"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ur_mesh.h"\n#include "ur_host.h"\n'
                   'int main() { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %u %u\\n", sizeof(ur_mesh_stream), sizeof(ur_mesh_primitive), sizeof(ur_mesh_section), '
                   'sizeof(ur_mesh_layout), sizeof(ur_mesh_info), offsetof(ur_mesh_primitive, color), offsetof(ur_mesh_primitive, index_offset), '
                   'offsetof(ur_mesh_primitive, mode), offsetof(ur_mesh_primitive, color_components), offsetof(ur_mesh_info, radius), '
                   'offsetof(ur_mesh_info, out_of_range_triangles), UR_MESH_BUILD_MAX_STREAM_OPS, UR_MESH_VERTEX_BYTES); return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.run([_cxx(), "-std=c++17", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [16, 112, 12, 16, 56, 64, 80, 96, 104, 36, 52, 14, 64]
    P, I = lib.MeshPrimitive, lib.MeshInfo
    assert [C.sizeof(lib.MeshStream), C.sizeof(P), C.sizeof(lib.MeshSection), C.sizeof(lib.MeshLayout), C.sizeof(I), P.color.offset, P.index_offset.offset, P.mode.offset,
            P.color_components.offset, I.radius.offset, I.out_of_range_triangles.offset, lib.UR_MESH_BUILD_MAX_STREAM_OPS, 64] == got


def test_symbols_declared_exported_and_bound(urlib):
    from unclerenderer_amd import assets, hostmath, hotpath, lib
    strip = lambda text: re.sub(r"/\*.*?\*/", "", text, flags=re.S)  # noqa: E731
    for name, header in NEW.items():
        assert re.search(r"\b%s\s*\(" % name, strip((ROOT / "include" / header).read_text())), name
        assert name in lib.SIGNATURES and getattr(urlib, name) is not None
    assert callable(hotpath.HotPath.build_mesh) and callable(hotpath.mesh_draws) and callable(hostmath.mesh_build) and callable(assets.load_gltf_meshes)
    assert "mesh" not in strip((ROOT / "include" / "ur_frame.h").read_text())  # nothing is wired into the frame


def test_the_host_unit_builds_with_the_plain_compiler_and_builds_the_same(tmp_path, urlib):
    so = tmp_path / "libmesh_host.so"
    subprocess.run([_cxx(), "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", str(CSRC / "mesh_host.cpp"), "-o", str(so)], check=True)
    plain = C.CDLL(str(so))
    from unclerenderer_amd import hostmath, lib
    data, prims = M.case("soup")
    records = M.host_primitives(prims)
    vertices, indices, _, info = M.expected("soup")
    buf = np.frombuffer(data, np.uint8)
    hv, hi, hinfo = np.zeros_like(vertices), np.zeros_like(indices), lib.MeshInfo()
    rc = plain.ur_host_mesh_build(C.c_void_p(buf.ctypes.data), C.c_uint64(buf.size), hostmath.mesh_primitive_array(records), C.c_uint32(len(records)),
                                  C.c_void_p(hv.ctypes.data), C.c_void_p(hi.ctypes.data), None, C.byref(hinfo))
    assert rc == 0 and np.array_equal(hv, vertices) and np.array_equal(hi, indices) and bytes(hinfo) == R.info_bytes(info)


SANITIZE_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "ur_host.h"
// argv[1]: a file of { u64 buffer bytes, u32 n, u32 pad, n primitives, the buffer }. The buffers are exactly as long as the layout says,
// on the heap, so that a read or write past them is seen.
int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    unsigned long long size = 0; unsigned n = 0, pad = 0;
    if (fread(&size, 8, 1, f) != 1 || fread(&n, 4, 1, f) != 1 || fread(&pad, 4, 1, f) != 1) return 2;
    std::vector<ur_mesh_primitive> prims(n);
    if (fread(prims.data(), sizeof(ur_mesh_primitive), n, f) != n) return 2;
    unsigned char* buffer = (unsigned char*)malloc(size);
    if (fread(buffer, 1, size, f) != size) return 2;
    fclose(f);
    unsigned long long V = 0, I = 0;
    for (unsigned k = 0; k < n; ++k) { V += prims[k].vertex_count; I += prims[k].mode == 4 ? prims[k].index_count : 3ull * (prims[k].index_count - 2); }
    unsigned char* vertices = (unsigned char*)malloc(64 * V);
    uint32_t* indices = (uint32_t*)malloc(4 * I);
    ur_mesh_section* sections = (ur_mesh_section*)malloc(sizeof(ur_mesh_section) * n);
    ur_mesh_info info;
    int rc = ur_host_mesh_build(buffer, size, prims.data(), n, vertices, indices, sections, &info);
    unsigned long long sum = 0;
    for (unsigned long long i = 0; i < 64 * V; ++i) sum += vertices[i];
    for (unsigned long long i = 0; i < I; ++i) sum += indices[i];
    printf("%d %llu %u %u\n", rc, sum, info.normals_regenerated, info.tangents_regenerated);
    free(buffer); free(vertices); free(indices); free(sections);
    return rc == 0 ? 0 : 1;
}
"""


@pytest.mark.parametrize("name", ["soup", "modes_5121", "fans", "nan_bounds"])
def test_host_build_under_asan_and_ubsan(tmp_path, name):
    """A stand-alone program with its own main, csrc/mesh_host.cpp compiled in with -fsanitize=address,undefined: no Python, no device."""
    from unclerenderer_amd import hostmath
    main = tmp_path / "mesh_sanitize_main.cpp"
    main.write_text(SANITIZE_MAIN)
    exe = tmp_path / "mesh_sanitize"
    subprocess.run([_cxx(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", f"-I{ROOT / 'include'}", str(main),
                    str(CSRC / "mesh_host.cpp"), "-o", str(exe)], check=True)
    data, prims = M.case(name)
    records = M.host_primitives(prims)
    blob = tmp_path / "mesh.bin"
    blob.write_bytes(np.uint64(len(data)).tobytes() + np.uint32([len(records), 0]).tobytes() + b"".join(bytes(r) for r in records) + data)
    r = subprocess.run([str(exe), str(blob)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    vertices, indices, _, info = M.expected(name)
    total = int(vertices.view(np.uint8).sum(dtype=np.uint64)) + int(indices.sum(dtype=np.uint64))
    assert r.stdout.split() == ["0", str(total), str(info["normals_regenerated"]), str(info["tangents_regenerated"])]


def _prim(**kw):
    from unclerenderer_amd import hostmath
    base = dict(vertex_count=3, position=(0, 12), indices=(36, 3, 5125))
    base.update(kw)
    return hostmath.mesh_primitive(base.pop("vertex_count"), base.pop("position"), base.pop("indices"), **base)


def test_layout_refusals_and_sums(urlib):
    from unclerenderer_amd import hostmath, lib
    size = 48  # three positions and three u32 indices

    def refused(text, prim, buffer_size=size, n=1):
        layout = lib.MeshLayout()
        rc = urlib.ur_mesh_layout_of(hostmath.mesh_primitive_array([prim]), n, buffer_size, C.byref(layout), None)
        assert rc == lib.UR_EINVAL and text in urlib.ur_last_error().decode(), (text, rc, urlib.ur_last_error())

    refused("no primitives", _prim(), n=0)
    refused("POSITION reads past the buffer", _prim(), buffer_size=35)
    refused("POSITION reads past the buffer", _prim(position=(16, 12)), buffer_size=48)
    refused("NORMAL reads past the buffer", _prim(normal=(16, 12)))
    refused("TEXCOORD_0 reads past the buffer", _prim(texcoord=(28, 8)))
    refused("TANGENT reads past the buffer", _prim(tangent=(0, 20)))
    refused("COLOR_0 reads past the buffer", _prim(color=(12, 12), color_components=4))
    refused("the indices read past the buffer", _prim(indices=(40, 3, 5125)))
    refused("the indices read past the buffer", _prim(indices=(2 ** 40, 3, 5121)))
    refused("mode 3", _prim(mode=3))
    refused("mode 7", _prim(mode=7))
    refused("component type 5126", _prim(indices=(36, 3, 5126)))
    refused("a triangle list of 4 indices", _prim(indices=(32, 4, 5125)))
    refused("2 indices (at least 3)", _prim(indices=(36, 2, 5125), mode=5))
    refused("no vertices", _prim(vertex_count=0))
    refused("no POSITION", _prim(position=None))
    bad = _prim()
    bad.position.stride = 0
    refused("stride 0", bad)
    refused("stride 14", _prim(position=(0, 14)))
    refused("offset 2 is not 4-byte aligned", _prim(position=(2, 12)))
    refused("index offset 37 is not 4-byte aligned", _prim(indices=(37, 3, 5125)))
    refused("index offset 37 is not 2-byte aligned", _prim(indices=(37, 3, 5123)))
    refused("a colour of 5 components", _prim(color=(0, 12), color_components=5))
    many = _prim(vertex_count=2 ** 32 - 1, position=(0, 4))
    layout = lib.MeshLayout()
    assert urlib.ur_mesh_layout_of(hostmath.mesh_primitive_array([many, many]), 2, 2 ** 40, C.byref(layout), None) == lib.UR_EINVAL
    assert "2^32 - 1" in urlib.ur_last_error().decode()
    assert urlib.ur_mesh_layout_of(hostmath.mesh_primitive_array([_prim()]), 1, size, None, None) == lib.UR_EINVAL
    # the sums: a list of 9, a strip of 5 and a fan of 5
    data, prims = M.case("modes_5123")
    layout, sections = hostmath.mesh_layout(M.host_primitives(prims), len(data))
    assert (layout.vertex_count, layout.index_count) == (21, 27) and sections == [(0, 0, 9), (7, 9, 9), (14, 18, 9)] == M.expected("modes_5123")[2]
    assert layout.scratch_bytes % 16 == 0 and layout.scratch_bytes >= 256 + 3 * 128 + 4 * 21 + 4 * 27 + 37 * 9


def test_build_refusals_that_need_no_device(urlib):
    """Every check comes before the context is looked at: a stand-in context is enough, the addresses are numbers and none is dereferenced."""
    from unclerenderer_amd import hostmath, lib
    stand_in = C.create_string_buffer(4096)
    ctx, buffer, vertices, indices, scratch, info = C.addressof(stand_in), 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
    prims = hostmath.mesh_primitive_array([_prim()])
    layout = lib.MeshLayout()
    assert urlib.ur_mesh_layout_of(prims, 1, 48, C.byref(layout), None) == 0
    need = int(layout.scratch_bytes)

    def refused(text, *, c=ctx, b=buffer, size=48, p=prims, n=1, v=vertices, i=indices, s=scratch, sb=need, o=info):
        rc = urlib.ur_mesh_build(c, b, size, p, n, v, i, s, sb, o)
        assert rc == lib.UR_EINVAL and text in urlib.ur_last_error().decode(), (text, rc, urlib.ur_last_error())

    for name in ("c", "b", "v", "i", "s", "o"):
        refused("null", **{name: None})
    refused("no primitives", p=None)
    refused("no primitives", n=0)
    refused("past the buffer", size=40)
    refused("mode 9", p=hostmath.mesh_primitive_array([_prim(mode=9)]))
    refused("buffer not 4-byte aligned", b=buffer + 2)
    refused("vertices not 16-byte aligned", v=vertices + 8)
    refused("indices or info not 4-byte aligned", i=indices + 2)
    refused("indices or info not 4-byte aligned", o=info + 1)
    refused("scratch not 16-byte aligned", s=scratch + 4)
    refused("scratch bytes", sb=need - 1)
    refused("vertices and indices overlap", i=vertices + 64)
    refused("vertices and scratch overlap", s=vertices + 16)
    refused("vertices and info overlap", o=vertices + 188)
    refused("indices and scratch overlap", s=indices - 16)
    refused("vertices and buffer overlap", b=vertices + 4)
    refused("scratch and info overlap", o=scratch + need - 4)
    refused("info and buffer overlap", b=info + 4, size=48)


def test_python_routing(urlib, monkeypatch):
    from unclerenderer_amd import assets, hostmath, hotpath
    # a refused mesh is refused before anything is uploaded
    monkeypatch.setattr(hotpath.tensors, "to_device", lambda *args: pytest.fail("a refused mesh must not be uploaded"))

    class NoDevice(hotpath.HotPath):
        def __init__(self):
            self._L = urlib
    with pytest.raises(ValueError, match="past the buffer"):
        NoDevice().build_mesh(bytes(40), [_prim()])
    with pytest.raises(ValueError, match="mode 2"):
        hostmath.mesh_build(bytes(48), [_prim(mode=2)])
    # the loader's records are the restatement's reading of the file
    _, meshes, gltf = M.fixture("CompareNormal")
    for m, prims in enumerate(meshes):
        records, materials = assets.gltf_mesh_primitives(gltf, m)
        assert [bytes(r) for r in records] == [bytes(r) for r in M.host_primitives(prims)] and materials == R.gltf_primitives(gltf, m)[1]
    with pytest.raises(ValueError, match="embedded"):
        path = ROOT / "tests" / "golden" / "assets"
        import json
        import tempfile
        with tempfile.TemporaryDirectory() as d:
            p = __import__("pathlib").Path(d) / "e.gltf"
            p.write_text(json.dumps({"buffers": [{"uri": "data:application/octet-stream;base64,AAAA", "byteLength": 3}]}))
            assert path.exists()
            assets.read_gltf(p)
    with pytest.raises(ValueError, match="GLB"):
        with tempfile.TemporaryDirectory() as d:
            p = __import__("pathlib").Path(d) / "e.glb"
            p.write_bytes(b"glTF\x02\0\0\0")
            assets.read_gltf(p)

    # mesh_draws: one command per primitive, sections' start and count, base vertex 0, stride 64
    class T:
        pass
    mesh = hotpath.Mesh(T(), T(), [(0, 0, 9), (7, 9, 9)], None)
    draws = hotpath.mesh_draws(mesh, "c", 16, 608)
    assert [(d["start_index"], d["index_count"], d["base_vertex"], d["stride"], d["constants_offset"]) for d in draws] == [(0, 9, 0, 64, 16), (9, 9, 0, 64, 624)]
    assert all(d["vertices"] is mesh.vertices and d["indices"] is mesh.indices for d in draws)


def test_mesh_kernels_use_no_scratch_and_spill_nothing(urlib, tmp_path):
    from tests.code_objects import library_kernels
    kernels = {k: v for k, v in library_kernels(tmp_path).items() if re.search(r"mesh_\w+_kernel", k)}
    assert len(kernels) == 13, sorted(kernels)
    for name, meta in kernels.items():
        assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0 and meta["sgpr_spill_count"] == 0, (name, meta)
        assert meta["vgpr_count"] <= 64, (name, meta)
        print(name, meta["vgpr_count"], meta["sgpr_count"])
