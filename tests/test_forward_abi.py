"""The Forward pass without a GPU: the new symbols and struct of include/ur_raster.h, every argument check of ur_forward_pass that returns
before a device is touched, and the Python routing."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
LLVM = Path("/opt/rocm/lib/llvm/bin")
NEW = ("ur_forward_pass", "ur_forward_pass_parts")

VIEW = np.eye(4, dtype=np.float32).reshape(-1)
PROJ = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 0.125, 0], np.float32)


def _strip(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _c_compiler():
    for c in (shutil.which("cc"), shutil.which("gcc"), "/opt/rocm/lib/llvm/bin/clang", shutil.which("clang")):
        if c and Path(c).exists():
            return c
    return None


def test_symbols_declared_exported_and_bound(urlib):
    from unclerenderer_amd import hotpath, lib
    header = _strip((ROOT / "include" / "ur_raster.h").read_text())
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header) and name in lib.SIGNATURES and getattr(urlib, name) is not None
        decl = re.search(r"int %s\s*\((.*?)\);" % name, header, re.S).group(1)
        assert "const float* depth" not in decl and "float* depth" in decl and "const ur_forward_targets* targets" in decl
        assert "const ur_gbuffer_mask* mask" in decl and "const ur_scene_constants* frame_constants" in decl and "const ur_lighting_tables* tables" in decl
    parts = re.search(r"int ur_forward_pass_parts\s*\((.*?)\);", header, re.S).group(1)
    assert "uint32_t parts" in parts
    assert len(lib.SIGNATURES["ur_forward_pass"][1]) == 18 and len(lib.SIGNATURES["ur_forward_pass_parts"][1]) == 19
    assert callable(hotpath.HotPath.forward_pass) and callable(hotpath.forward_targets)
    if not (LLVM / "llvm-readelf").exists():
        pytest.skip("llvm tools not found")
    dyn = subprocess.run([str(LLVM / "llvm-readelf"), "--dyn-syms", "--wide", str(lib.library_path())], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert re.search(r"FUNC\s+GLOBAL\s+DEFAULT\s+\d+\s+%s$" % name, dyn, re.M), name


def test_struct_layout_matches_a_compiled_probe(tmp_path):
    from unclerenderer_amd import lib
    raster = (ROOT / "include" / "ur_raster.h").read_text()
    body = re.search(r"typedef struct ur_forward_targets \{(.*?)\} ur_forward_targets;", raster, re.S).group(1)
    names = [re.findall(r"(\w+)\s*$", d.strip())[0] for d in _strip(body).split(";") if d.strip()]
    K = lib.ForwardTargets
    assert names == [n for n, _ in K._fields_] == ["hdr", "keys"]
    cc = _c_compiler()
    assert cc is not None, "no C compiler to take sizeof(ur_forward_targets)"
    src = tmp_path / "s.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ur_raster.h"\nint main(void) { printf("%zu %zu %zu\\n", '
                   "sizeof(ur_forward_targets), offsetof(ur_forward_targets, hdr), offsetof(ur_forward_targets, keys)); return 0; }\n")
    exe = tmp_path / "s"
    subprocess.run([cc, "-std=c99", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(K), K.hdr.offset, K.keys.offset] == [16, 0, 8]


def test_argument_checks(urlib):
    """On an 8 x 8 frame over stand-in addresses 4096 bytes apart (nothing is dereferenced: every call returns before the context is used)."""
    from unclerenderer_amd import lib
    buf = (C.c_uint64 * 16384)()
    base = C.addressof(buf)
    ctx = C.c_void_p(base + 120000)
    E, U = lib.UR_EINVAL, lib.UR_EUNSUPPORTED
    depth, cmds, idx, cnt, st, hdr, keys, k64, mst, won, mats, other, shadow, cube, lut = (C.c_void_p(base + 4096 * k) for k in range(1, 16))
    v, p = lib.fptr(VIEW), lib.fptr(PROJ)
    off = lambda q, k: C.c_void_p(q.value + k)  # noqa: E731
    err = lambda: urlib.ur_last_error().decode()  # noqa: E731
    texels = urlib.ur_env_cube_texels(2, 2)  # 6 * (16 + 9) bordered texels and their row pairs: 2448 bytes, inside its 4096
    assert 0 < texels * 8 <= 4096

    def draws(**kw):
        d = lib.RasterDraws(cmds, 4, None, None, 0, None)
        for k, val in kw.items():
            setattr(d, k, val)
        return d

    def targets(**kw):
        t = lib.ForwardTargets(hdr, keys)
        for k, val in kw.items():
            setattr(t, k, val)
        return t

    def scene(**kw):
        s = lib.SceneConstants()
        s.ShadowStrength, s.ShadowMapSize[0], s.ShadowMapSize[1], s.EnvMapMipCount = 0.5, 4.0, 4.0, 2.0
        for k, val in kw.items():
            setattr(s, k, val)
        return s

    def tables(**kw):
        t = lib.LightingTables(shadow, cube, 2, 2, lut, 8, 4, texels)
        for k, val in kw.items():
            setattr(t, k, val)
        return t

    keep = []

    def mask(d=None, **kw):
        d = draws() if d is None else d
        keep.append(d)
        m = lib.GBufferMask(C.pointer(d), k64, mst, won)
        for k, val in kw.items():
            setattr(m, k, val)
        return m

    def call(ctx_=ctx, d=None, depth_=depth, t="default", w=8, h=8, row0=0, rows=8, flags=0, bits=0, m="default", mt=mats, parts=None, s="default", tb="default"):
        d = draws() if d is None else d
        t = targets() if isinstance(t, str) else t
        m = mask() if isinstance(m, str) else m
        s = scene() if isinstance(s, str) else s
        tb = tables() if isinstance(tb, str) else tb
        ref = lambda x: C.byref(x) if x is not None else None  # noqa: E731
        head = (ctx_, v, p, C.byref(d), depth_, ref(t), w, h, row0, rows, flags, bits, st)
        tail = (mt, 4, ref(m), ref(s), ref(tb))
        return urlib.ur_forward_pass(*head, *tail) if parts is None else urlib.ur_forward_pass_parts(*head, parts, *tail)

    # the GBuffer cases, with and without a mask
    for m in ("default", None):
        assert call(ctx_=None, m=m) == E and call(depth_=None, m=m) == E and call(rows=0, m=m) == E and call(row0=8, rows=1, m=m) == E
        assert call(flags=2, m=m) == E and "flag" in err()
        assert call(bits=32, m=m) == E and call(mt=off(mats, 8), m=m) == E and "material" in err()
        assert call(d=draws(visible_idx=idx), m=m) == E and call(d=draws(commands=off(cmds, 8)), m=m) == E
        assert "ur_forward_pass" in err()
        assert call(d=draws(command_count=1 << 24, commands=cmds), m=None) == U
        # the targets
        assert call(t=None, m=m) == E and call(t=targets(hdr=None), m=m) == E and call(t=targets(keys=None), m=m) == E and "null" in err()
        assert call(t=targets(hdr=off(hdr, 4)), m=m) == E and call(t=targets(keys=off(keys, 2)), m=m) == E and "misaligned" in err()
        # the frame constants and the tables
        assert call(s=None, m=m) == E and "frame_constants" in err()
        assert call(tb=None, m=m) == E and "tables" in err()
        assert call(tb=tables(shadow_map=None), m=m) == E and "ShadowStrength" in err()
        assert call(s=scene(ShadowMapSize=(C.c_float * 2)(0.0, 4.0)), m=m) == E and call(s=scene(ShadowMapSize=(C.c_float * 2)(4.0, 20000.0)), m=m) == E
        assert call(s=scene(ShadowMapSize=(C.c_float * 2)(float("nan"), 4.0)), m=m) == E and "ShadowMapSize" in err()
        assert call(tb=tables(env_cube_texels=texels - 1), m=m) == E and "env_cube_texels" in err()
        assert call(tb=tables(env_cube_texels=6 * 25), m=m) == E  # an earlier layout's tag: the bordered faces alone
        for field, zero in (("env_base_size", 0), ("env_mip_count", 0), ("lut_width", 0), ("lut_height", 0), ("env_cube", None), ("brdf_lut_rg16", None)):
            assert call(tb=tables(**{field: zero}), m=m) == E and "tables" in err(), field
        assert call(tb=tables(env_mip_count=17), m=m) == E
        # hdr (512 bytes) or keys (256) over an input, from either side
        inputs = ((depth, 256), (cmds, 256), (mats, 320), (shadow, 64), (cube, texels * 8), (lut, 128))
        for q, size in inputs:
            assert call(t=targets(hdr=off(q, size - 8)), m=m) == E and "overlaps" in err(), size
            assert call(t=targets(hdr=off(q, -504)), m=m) == E and "overlaps" in err(), size
            assert call(t=targets(keys=off(q, size - 4)), m=m) == E and "overlaps" in err(), size
            assert call(t=targets(keys=off(q, -252)), m=m) == E and "overlaps" in err(), size
        assert call(t=targets(keys=off(hdr, 508)), m=m) == E and call(t=targets(keys=off(hdr, -252)), m=m) == E and "overlaps" in err()
    # a shadow map that is not used may be null, and is then no input
    assert call(s=scene(ShadowStrength=0.0), tb=tables(shadow_map=None), m=mask(keys64=None)) == E and "keys64" in err()
    # the masked selection's cases
    assert call(m=mask(draws=None)) == E and "mask" in err()
    assert call(m=mask(keys64=None)) == E and call(m=mask(keys64=off(k64, 4))) == E and "keys64" in err()
    assert call(m=mask(draws(commands=other))) == E and call(m=mask(draws(command_count=3))) == E
    assert call(m=mask(keys64=off(hdr, 504))) == E and call(m=mask(keys64=off(keys, -504))) == E and call(m=mask(keys64=off(depth, 248))) == E and "overlaps" in err()
    # the parts word: 0 and unknown bits are refused, and every check holds in either part
    for bad in (0, 4, 0x80000001):
        assert call(parts=bad) == E and "parts" in err() and call(parts=bad, m=None) == E
    for part in (1, 2, 3):
        assert call(parts=part, s=None) == E and call(parts=part, tb=None) == E and call(parts=part, t=targets(hdr=None)) == E
        assert call(parts=part, m=mask(keys64=None)) == E
    del buf


class _FakeTensor:
    def __init__(self, dtype, n, at):
        self.dtype, self._n, self._at, self.is_cuda = dtype, n, at, True

    def is_contiguous(self):
        return True

    def numel(self):
        return self._n

    def element_size(self):
        return 4

    def data_ptr(self):
        return self._at


def test_python_routing():
    """HotPath.forward_pass goes to ur_forward_pass, or to ur_forward_pass_parts when parts is given, with or without a mask and
    materials, and hands over the scene and the tables."""
    import torch
    from unclerenderer_amd import hotpath as hp
    from unclerenderer_amd import lib
    called = []

    class L:
        def __getattr__(self, name):
            def f(*args):
                called.append((name, args))
                return lib.UR_OK
            return f

    class Self:
        _L, _ctx = L(), C.c_void_p(1)

    t = lambda dtype, n, at: _FakeTensor(dtype, n, at)  # noqa: E731
    depth, cmds, keys64 = t(torch.float32, 64, 0x1000), t(torch.int32, 64, 0x2000), t(torch.int64, 64, 0x3000)
    tg = hp.forward_targets(t(torch.float16, 256, 0x5000), t(torch.int32, 64, 0x6000))
    assert tg.hdr == 0x5000 and tg.keys == 0x6000
    mask_draws = hp.raster_draws(cmds)
    table = t(torch.int32, 80, 0x4000)
    scene, tables = lib.SceneConstants(), lib.LightingTables()
    scene.LightIntensity, tables.lut_width = 7.0, 128
    common = (Self(), VIEW, PROJ, cmds, depth, tg, 8, 8)
    hp.HotPath.forward_pass(*common, scene=scene, tables=tables)
    hp.HotPath.forward_pass(*common, scene=scene, tables=tables, materials=(table, 4), mask_draws=mask_draws, keys64=keys64)
    hp.HotPath.forward_pass(*common, scene=scene, tables=tables, parts=lib.UR_GBUFFER_PART_RESOLVE)
    assert [name for name, _ in called] == ["ur_forward_pass", "ur_forward_pass", "ur_forward_pass_parts"]
    plain, masked, parts = (args for _, args in called)
    assert plain[13] is None and plain[14] == 0 and plain[15] is None
    assert C.cast(plain[16], C.POINTER(lib.SceneConstants)).contents.LightIntensity == 7.0
    assert C.cast(plain[17], C.POINTER(lib.LightingTables)).contents.lut_width == 128
    assert masked[13].value == 0x4000 and masked[14] == 4
    m = C.cast(masked[15], C.POINTER(lib.GBufferMask)).contents
    assert m.keys64 == 0x3000 and m.stats6 is None and m.won is None and m.draws.contents.commands == 0x2000
    assert parts[13] == lib.UR_GBUFFER_PART_RESOLVE and parts[14] is None and parts[15] == 0 and parts[16] is None
    with pytest.raises(AssertionError):
        hp.HotPath.forward_pass(*common, scene=scene, tables=tables, mask_draws=mask_draws)  # no keys64
    with pytest.raises(TypeError):
        hp.HotPath.forward_pass(*common)  # scene and tables are required
