"""The alpha-masked GBuffer pass without a GPU: the new symbols and struct of include/ur_raster.h, the material bit, every argument check
of ur_gbuffer_pass_masked that returns before a device is touched, and the Python routing."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
LLVM = Path("/opt/rocm/lib/llvm/bin")
NEW = ("ur_gbuffer_pass_masked", "ur_gbuffer_pass_masked_parts")

VIEW = np.eye(4, dtype=np.float32).reshape(-1)
PROJ = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 0.125, 0], np.float32)


def _strip(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_symbols_declared_exported_and_bound(urlib):
    from unclerenderer_amd import lib
    header = _strip((ROOT / "include" / "ur_raster.h").read_text())
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header) and name in lib.SIGNATURES and getattr(urlib, name) is not None
    # the earlier entry points keep their signatures: depth stays const in them, and only the new ones take a mask
    for name in ("ur_gbuffer_pass", "ur_gbuffer_pass_parts", "ur_gbuffer_pass_materials", "ur_gbuffer_pass_materials_parts"):
        decl = re.search(r"int %s\s*\((.*?)\);" % name, header, re.S).group(1)
        assert "const float* depth" in decl and "mask" not in decl, name
    for name in NEW:
        decl = re.search(r"int %s\s*\((.*?)\);" % name, header, re.S).group(1)
        assert "const float* depth" not in decl and "float* depth" in decl and "const ur_gbuffer_mask* mask" in decl, name
    if not (LLVM / "llvm-readelf").exists():
        pytest.skip("llvm tools not found")
    dyn = subprocess.run([str(LLVM / "llvm-readelf"), "--dyn-syms", "--wide", str(lib.library_path())], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert re.search(r"FUNC\s+GLOBAL\s+DEFAULT\s+\d+\s+%s$" % name, dyn, re.M), name


def test_struct_layout_and_the_material_bit_match_the_header():
    from unclerenderer_amd import lib
    raster = (ROOT / "include" / "ur_raster.h").read_text()
    body = re.search(r"typedef struct ur_gbuffer_mask \{(.*?)\} ur_gbuffer_mask;", raster, re.S).group(1)
    names = [re.findall(r"(\w+)\s*$", d.strip())[0] for d in _strip(body).split(";") if d.strip()]
    K = lib.GBufferMask
    assert names == [n for n, _ in K._fields_] == ["draws", "keys64", "stats6", "won"]
    assert [getattr(K, n).offset for n, _ in K._fields_] == [0, 8, 16, 24] and C.sizeof(K) == 32
    assert int(re.search(r"#define UR_MATERIAL_ALPHA_MASK \(0x([0-9a-f]+)u\)", raster).group(1), 16) == lib.UR_MATERIAL_ALPHA_MASK == 0x10
    assert lib.UR_MATERIAL_ALPHA_MASK & (lib.UR_MATERIAL_NORMAL_MAP | lib.UR_MATERIAL_METALLIC_ROUGHNESS_MAP | lib.UR_MATERIAL_BASE_COLOR_MAP | lib.UR_MATERIAL_EMISSIVE_MAP) == 0


def test_argument_checks(urlib):
    """On an 8 x 8 frame over stand-in addresses 4096 bytes apart (nothing is dereferenced: every call returns before the context is used)."""
    from unclerenderer_amd import lib
    buf = (C.c_uint64 * 16384)()
    base = C.addressof(buf)
    ctx = C.c_void_p(base + 120000)
    E, U = lib.UR_EINVAL, lib.UR_EUNSUPPORTED
    depth, cmds, idx, cnt, st, a, b, c, hdr, oid, keys, k64, mst, won, mats, other = (C.c_void_p(base + 4096 * k) for k in range(1, 17))
    v, p = lib.fptr(VIEW), lib.fptr(PROJ)
    off = lambda q, k: C.c_void_p(q.value + k)  # noqa: E731
    err = lambda: urlib.ur_last_error().decode()  # noqa: E731

    def draws(**kw):
        d = lib.RasterDraws(cmds, 4, None, None, 0, None)
        for k, val in kw.items():
            setattr(d, k, val)
        return d

    def targets(**kw):
        t = lib.GBufferTargets(a, b, c, hdr, None, keys)
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

    def call(f=urlib.ur_gbuffer_pass_masked, ctx_=ctx, d=None, depth_=depth, t=None, w=8, h=8, row0=0, rows=8, flags=0, bits=0, m="default", mt=mats, parts=None):
        d = draws() if d is None else d
        t = targets() if t is None else t
        m = mask() if isinstance(m, str) else m
        head = (ctx_, v, p, C.byref(d), depth_, C.byref(t), w, h, row0, rows, flags, bits, st)
        tail = (mt, 4, C.byref(m) if m is not None else None)
        return f(*head, *tail) if parts is None else urlib.ur_gbuffer_pass_masked_parts(*head, parts, *tail)

    # ur_gbuffer_pass_materials' cases for the opaque selection, with and without a mask
    for m in ("default", None):
        assert call(ctx_=None, m=m) == E and call(depth_=None, m=m) == E and call(rows=0, m=m) == E and call(row0=8, rows=1, m=m) == E
        assert call(flags=2, m=m) == E and "flag" in err()
        assert call(bits=32, m=m) == E and call(t=targets(gbuf_a=None), m=m) == E and call(mt=off(mats, 8), m=m) == E and "material" in err()
        assert call(d=draws(visible_idx=idx), m=m) == E and call(d=draws(commands=off(cmds, 8)), m=m) == E
        assert "ur_gbuffer_pass_masked" in err()
    # ... and for the masked selection
    assert call(m=mask(draws=None)) == E and "mask" in err()
    assert call(m=mask(draws(visible_idx=idx))) == E and call(m=mask(draws(visible_count=cnt))) == E
    rg = lib.DrawRanges(idx, 2, cmds, cnt)
    assert call(m=mask(draws(visible_idx=idx, visible_count=cnt, ranges=C.pointer(rg)))) == E
    assert call(m=mask(draws(commands=None, ranges=C.pointer(lib.DrawRanges(idx, 0, cmds, cnt))))) == E
    assert call(m=mask(stats6=off(mst, 2))) == E and "misaligned" in err()
    # keys64, won
    assert call(m=mask(keys64=None)) == E and "keys64" in err()
    assert call(m=mask(keys64=off(k64, 4))) == E and "keys64" in err()
    assert call(m=mask(won=off(won, 2))) == E
    # one key space: the same commands and command_count
    assert call(m=mask(draws(commands=other))) == E and "key" in err()
    assert call(m=mask(draws(command_count=3))) == E and "command_count" in err()
    assert call(m=mask(draws(commands=None, ranges=C.pointer(lib.DrawRanges(idx, 2, other, cnt))))) == E
    # keys64 (8 x 8 x 8 = 512 bytes) over a target (gbuf_a 512 bytes, gbuf_c and keys 256) or depth (256 bytes), from either side
    for q, size in ((a, 512), (b, 512), (hdr, 512), (c, 256), (keys, 256), (depth, 256)):
        assert call(m=mask(keys64=off(q, size - 8))) == E and "overlaps" in err(), (q, size)
        assert call(m=mask(keys64=off(q, -504))) == E and "overlaps" in err(), (q, size)
    # ObjectId beside a mask is unsupported; without a mask it is ur_gbuffer_pass_materials' optional target
    assert call(t=targets(object_id=oid)) == U and "object_id" in err()
    assert call(t=targets(object_id=oid), m=mask(keys64=None)) == E  # (the argument errors come first)
    # the parts word
    for bad in (0, 4, 0x80000001):
        assert call(parts=bad) == E and "parts" in err()
    for part in (1, 2, 3):
        assert call(parts=part, m=mask(keys64=None)) == E and call(parts=part, t=targets(object_id=oid)) == U
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
    """HotPath.gbuffer_pass goes to ur_gbuffer_pass_masked(_parts) exactly when mask_draws is given, with materials or without, and
    pack_materials takes keys up to 31."""
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
    tg = lib.GBufferTargets()
    mask_draws = hp.raster_draws(cmds)
    table = t(torch.int32, 80, 0x4000)
    common = (Self(), VIEW, PROJ, cmds, depth, tg, 8, 8)
    hp.HotPath.gbuffer_pass(*common)
    hp.HotPath.gbuffer_pass(*common, materials=(table, 4))
    hp.HotPath.gbuffer_pass(*common, materials=(table, 4), mask_draws=mask_draws, keys64=keys64)
    hp.HotPath.gbuffer_pass(*common, mask_draws=mask_draws, keys64=keys64, parts=lib.UR_GBUFFER_PART_RASTER)
    assert [name for name, _ in called] == ["ur_gbuffer_pass", "ur_gbuffer_pass_materials", "ur_gbuffer_pass_masked", "ur_gbuffer_pass_masked_parts"]
    args = called[2][1]
    assert args[13].value == 0x4000 and args[14] == 4
    m = C.cast(args[15], C.POINTER(lib.GBufferMask)).contents
    assert m.keys64 == 0x3000 and m.stats6 is None and m.won is None and m.draws.contents.commands == 0x2000
    assert called[3][1][13] == lib.UR_GBUFFER_PART_RASTER and called[3][1][14] is None and called[3][1][15] == 0
    with pytest.raises(AssertionError):
        hp.HotPath.gbuffer_pass(*common, mask_draws=mask_draws)  # no keys64
    with pytest.raises(AssertionError):
        hp.pack_materials([{"key": 32}])
