"""The textured GBuffer pass without a GPU: the new symbols (ur_gbuffer_pass_materials[_parts] in include/ur_raster.h, the two host tables,
ur_frame_set_gbuffer_materials) are declared, exported and bound; ur_material and ur_texture2d match the header; every argument check
returns before the context is used."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
LLVM = Path("/opt/rocm/llvm/bin")
NEW = ("ur_gbuffer_pass_materials", "ur_gbuffer_pass_materials_parts", "ur_host_srgb_decode_table", "ur_host_lod_table", "ur_frame_set_gbuffer_materials")

VIEW = np.eye(4, dtype=np.float32).reshape(-1)
PROJ = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 0.125, 0], np.float32)


def _strip(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_symbols_declared_exported_and_bound(urlib):
    from unclerenderer_amd import hostmath, lib
    from unclerenderer_amd import hotpath as hp
    raster, frame, host = (_strip((ROOT / "include" / n).read_text()) for n in ("ur_raster.h", "ur_frame.h", "ur_host.h"))
    assert re.search(r"\bur_gbuffer_pass_materials\s*\(", raster) and re.search(r"\bur_gbuffer_pass_materials_parts\s*\(", raster)
    assert re.search(r"\bur_frame_set_gbuffer_materials\s*\(", frame)
    assert re.search(r"\bur_host_srgb_decode_table\s*\(", host) and re.search(r"\bur_host_lod_table\s*\(", host)
    for name in NEW:
        assert name in lib.SIGNATURES and getattr(urlib, name) is not None
    assert callable(hp.pack_texture) and callable(hp.pack_materials) and callable(hp.Frame.set_gbuffer_materials)
    assert callable(hostmath.lod_table) and callable(hostmath.srgb_decode_table)
    assert hostmath.lod_table().shape == (127,) and hostmath.srgb_decode_table().shape == (256,)
    if not (LLVM / "llvm-readelf").exists():
        pytest.skip("llvm tools not found")
    dyn = subprocess.run([str(LLVM / "llvm-readelf"), "--dyn-syms", "--wide", str(lib.library_path())], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert re.search(r"FUNC\s+GLOBAL\s+DEFAULT\s+\d+\s+%s$" % name, dyn, re.M), name


def _names(header, struct):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, re.S).group(1)
    return [n for d in _strip(body).split(";") if d.strip() for n in re.findall(r"(\w+)(?:\[\d+\])?\s*(?:,|$)", d.strip().split(None, 1)[1])]


def test_struct_layout_and_constants_match_the_header():
    from unclerenderer_amd import lib
    raster = (ROOT / "include" / "ur_raster.h").read_text()
    T, M = lib.Texture2D, lib.Material
    assert _names(raster, "ur_texture2d") == [n for n, _ in T._fields_] == ["texels", "width", "height", "mips", "format", "reserved"]
    assert [getattr(T, n).offset for n, _ in T._fields_] == [0, 8, 10, 12, 13, 14] and C.sizeof(T) == 16
    assert _names(raster, "ur_material") == [n for n, _ in M._fields_] == ["base_color", "metallic_roughness", "normal", "emissive", "pipeline_key", "reserved"]
    assert [getattr(M, n).offset for n, _ in M._fields_] == [0, 16, 32, 48, 64, 68] and C.sizeof(M) == 80
    defined = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (UR_TEXTURE_\w+) (\d+)u", raster)}
    assert defined == {"UR_TEXTURE_R8G8B8A8_UNORM": 28, "UR_TEXTURE_R8G8B8A8_UNORM_SRGB": 29}
    assert (lib.UR_TEXTURE_R8G8B8A8_UNORM, lib.UR_TEXTURE_R8G8B8A8_UNORM_SRGB) == (28, 29)
    bits = {m.group(1): int(m.group(2), 16) for m in re.finditer(r"#define (UR_MATERIAL_\w+) 0x([0-9a-f]+)u", raster)}
    assert bits == {"UR_MATERIAL_NORMAL_MAP": 1, "UR_MATERIAL_METALLIC_ROUGHNESS_MAP": 2, "UR_MATERIAL_BASE_COLOR_MAP": 4, "UR_MATERIAL_EMISSIVE_MAP": 8}
    for k, v in bits.items():
        assert getattr(lib, k) == v


def test_argument_checks(urlib):
    """ur_gbuffer_pass' checks in both new entry points, the table's alignment, and a NULL table taken as ur_gbuffer_pass (no complaint
    about it: the call fails on the argument that is wrong)."""
    from unclerenderer_amd import lib
    buf = (C.c_uint64 * 16384)()
    base = C.addressof(buf)
    ctx = C.c_void_p(base + 120000)  # never dereferenced: every check below returns before it is used
    E = lib.UR_EINVAL
    depth, cmds, idx, cnt, st, a, b, c, hdr, oid, keys, mats = (C.c_void_p(base + 4096 * k) for k in range(1, 13))
    v, p = lib.fptr(VIEW), lib.fptr(PROJ)
    off = lambda q, k: C.c_void_p(q.value + k)  # noqa: E731
    ok = lib.RasterDraws(cmds, 4, None, None, 0, None)
    tg = lib.GBufferTargets(a, b, c, hdr, oid, keys)
    whole = lambda m=mats, n=4, ctx_=ctx, v_=v, d=ok, depth_=depth, t=tg, w=64, rows=64, flags=0, bits=0, st_=st: \
        urlib.ur_gbuffer_pass_materials(ctx_, v_, p, C.byref(d) if d is not None else None, depth_, C.byref(t) if t is not None else None, w, 64, 0, rows, flags, bits, st_, m, n)  # noqa: E731
    parts = lambda part, m=mats, n=4, rows=64, t=tg: \
        urlib.ur_gbuffer_pass_materials_parts(ctx, v, p, C.byref(ok), depth, C.byref(t), 64, 64, 0, rows, 0, 0, st, part, m, n)  # noqa: E731
    for m in (mats, None):
        assert whole(m, ctx_=None) == E and "null" in urlib.ur_last_error().decode()
        assert whole(m, v_=None) == E and whole(m, d=None) == E and whole(m, depth_=None) == E and whole(m, t=None) == E
        assert whole(m, w=0) == E and whole(m, w=16385) == E and whole(m, rows=0) == E and whole(m, rows=65) == E
        assert whole(m, flags=2) == E and "flag" in urlib.ur_last_error().decode()
        assert whole(m, bits=32) == E and "key_triangle_bits" in urlib.ur_last_error().decode()
        assert whole(m, depth_=off(depth, 2)) == E and whole(m, st_=off(st, 1)) == E
        assert whole(m, t=lib.GBufferTargets(a, b, c, hdr, oid, None)) == E and whole(m, t=lib.GBufferTargets(off(a, 4), b, c, hdr, oid, keys)) == E
        assert whole(m, d=lib.RasterDraws(cmds, 1 << 24, None, None, 0, None)) == lib.UR_EUNSUPPORTED
        for bad in (0, 4, 0x80000001):
            assert parts(bad, m) == E and "parts" in urlib.ur_last_error().decode()
        for part in (1, 2, 3):
            assert parts(part, m, rows=0) == E and parts(part, m, t=lib.GBufferTargets(None, b, c, hdr, oid, keys)) == E
    # the errors name the entry point that was called
    assert whole(rows=0) == E and urlib.ur_last_error().decode().startswith("ur_gbuffer_pass_materials:")
    assert whole(w=0) == E and urlib.ur_last_error().decode().startswith("ur_gbuffer_pass_materials:")
    assert parts(3, rows=0) == E and urlib.ur_last_error().decode().startswith("ur_gbuffer_pass_materials:")
    assert parts(0) == E and urlib.ur_last_error().decode().startswith("ur_gbuffer_pass_materials_parts:")
    assert urlib.ur_gbuffer_pass(ctx, v, p, C.byref(ok), depth, C.byref(tg), 64, 64, 0, 0, 0, 0, st) == E and urlib.ur_last_error().decode().startswith("ur_gbuffer_pass:")
    for by in (4, 8, 12):
        assert whole(off(mats, by)) == E and "material" in urlib.ur_last_error().decode()
        for part in (1, 2, 3):
            assert parts(part, off(mats, by)) == E and "material" in urlib.ur_last_error().decode()
    # a NULL table with a misaligned-looking count is not looked at: the error is the other argument's
    assert whole(None, 0xFFFFFFFF, rows=0) == E and "rows" in urlib.ur_last_error().decode()
    # the frame setter
    f = urlib.ur_frame_set_gbuffer_materials
    assert f(None, mats, 4) == E and "null frame" in urlib.ur_last_error().decode()
    assert f(None, None, 0) == E
    frame = C.c_void_p(base + 64)  # never dereferenced by the check below
    assert f(frame, off(mats, 8), 4) == E and "misaligned" in urlib.ur_last_error().decode()
    del buf
