"""The ObjectId pass and the pick without a GPU: the new symbols and struct of include/ur_raster.h, every argument check of ur_object_id_pass
and ur_object_id_pick that returns before a device is touched, the empty pick, the new kernels' metadata, and the Python routing."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
LLVM = Path("/opt/rocm/lib/llvm/bin")
NEW = ("ur_object_id_pass", "ur_object_id_pick")

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
        decl = re.search(r"int %s\s*\((.*?)\);" % name, header, re.S).group(1)
        assert "const float* depth" in decl and name in lib.SIGNATURES and getattr(urlib, name) is not None
        assert len(lib.SIGNATURES[name][1]) == decl.count(",") + 1, name
    assert len(lib.SIGNATURES["ur_object_id_pass"][1]) == 14 and len(lib.SIGNATURES["ur_object_id_pick"][1]) == 13
    assert hotpath.HotPath.object_id_pass is not None and hotpath.HotPath.object_id_pick is not None
    # the masked pass keeps its return value for an ObjectId target and now says where to go
    comment = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int ur_gbuffer_pass_masked\(", (ROOT / "include" / "ur_raster.h").read_text(), re.S).group(1)
    assert "UR_EUNSUPPORTED" in comment and "ur_object_id_pass" in comment
    if not (LLVM / "llvm-readelf").exists():
        pytest.skip("llvm tools not found")
    dyn = subprocess.run([str(LLVM / "llvm-readelf"), "--dyn-syms", "--wide", str(lib.library_path())], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert re.search(r"FUNC\s+GLOBAL\s+DEFAULT\s+\d+\s+%s$" % name, dyn, re.M), name


def test_struct_layout_matches_a_compiled_probe(tmp_path):
    from unclerenderer_amd import lib
    raster = (ROOT / "include" / "ur_raster.h").read_text()
    body = re.search(r"typedef struct ur_pick_result \{(.*?)\} ur_pick_result;", raster, re.S).group(1)
    names = [re.findall(r"(\w+)\s*$", d.strip())[0] for d in _strip(body).split(";") if d.strip()]
    K = lib.PickResult
    assert names == [n for n, _ in K._fields_] == ["object_id", "key", "slot", "depth_bits"]
    assert int(re.search(r"#define UR_PICK_MAX_POINTS (\d+)u", raster).group(1)) == lib.UR_PICK_MAX_POINTS == 64
    cc = _c_compiler()
    assert cc is not None, "no C compiler to take sizeof(ur_pick_result)"
    src = tmp_path / "s.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ur_raster.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %u\\n", sizeof(ur_pick_result), '
                   "offsetof(ur_pick_result, object_id), offsetof(ur_pick_result, key), offsetof(ur_pick_result, slot), offsetof(ur_pick_result, depth_bits), "
                   "UR_PICK_MAX_POINTS); return 0; }\n")
    exe = tmp_path / "s"
    subprocess.run([cc, "-std=c99", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(K), K.object_id.offset, K.key.offset, K.slot.offset, K.depth_bits.offset, 64] == [16, 0, 4, 8, 12, 64]


def test_new_kernels_use_no_scratch_and_the_keyed_raster_keeps_its_registers(urlib, tmp_path):
    """The code objects' metadata notes: pick_kernel in both forms, pick_finish_kernel and object_id_resolve_kernel have no
    scratch and spill no VGPR, the pick within the raster's own occupancy step; raster_kernel<VisPolicy<...>>, whose walk and per-triangle
    front half pick_kernel shares (csrc/raster_front.h), stays without scratch inside its four-wave step (3.16 records the counts)."""
    from tests.code_objects import library_kernels
    kernels = library_kernels(tmp_path)
    find = lambda pattern: {k: m for k, m in kernels.items() if re.search(pattern, k)}  # noqa: E731
    picks = find(r"\d+pick_kernelINS_9VisPolicyILb[01]E+v")
    assert len(picks) == 2, sorted(picks)
    new = {**picks, **find(r"\d+pick_finish_kernelE"), **find(r"\d+object_id_resolve_kernelE")}
    assert len(new) == 4, sorted(new)
    for name, m in new.items():
        print(name, m)
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
    rasters = find(r"\d+raster_kernelINS_9VisPolicyILb[01]E+v")
    assert len(rasters) == 2, sorted(rasters)
    for name, m in rasters.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["vgpr_count"] <= 128, (name, m)
    assert all(m["vgpr_count"] <= 128 for m in picks.values()), picks  # four waves per SIMD, as the raster


# The VGPR count up to which a kernel keeps the waves per SIMD it had before it shared csrc/raster_front.h (512 / waves, in granules of 8)
OCCUPANCY_STEP = {
    r"\d+raster_kernelINS_12ShadowPolicyEE": 96,          # 5 waves (it had 87)
    r"\d+raster_kernelINS_11DepthPolicyILb[01]EE": 128,   # 4 waves (104 and 110)
    r"\d+raster_kernelINS_9VisPolicyILb[01]EE": 128,      # 4 waves (114 and 120)
    r"\d+raster_kernelINS_10MaskPolicyILb[01]EE": 256,    # 2 waves (220)
    r"\d+pick_kernelINS_9VisPolicyILb[01]EE": 80,         # 6 waves (79)
}


def test_the_kernels_over_the_shared_front_half_keep_their_occupancy_step(urlib, tmp_path):
    """raster_kernel in its seven forms and pick_kernel in both are one walk and one per-triangle front half (csrc/raster_front.h) plus
    their own back halves: none has scratch or spills a VGPR, and each stays at or below the VGPR count of the occupancy step it had when
    pick_kernel carried its own copy (DESIGN.md 3.16 has the counts). Metadata notes only; spilled SGPRs move with any change and are not held."""
    from tests.code_objects import library_kernels
    kernels = library_kernels(tmp_path)
    seen = 0
    for pattern, bound in OCCUPANCY_STEP.items():
        found = {k: m for k, m in kernels.items() if re.search(pattern, k)}
        assert len(found) == (1 if "Shadow" in pattern else 2), (pattern, sorted(found))
        for name, m in found.items():
            print(name, m)
            assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["vgpr_count"] <= bound, (name, m, bound)
        seen += len(found)
    assert seen == 9


def test_argument_checks(urlib):
    """On an 8 x 8 frame over stand-in addresses 4096 bytes apart (nothing is dereferenced: every call returns before the context is used)."""
    from unclerenderer_amd import lib
    buf = (C.c_uint64 * 16384)()
    base = C.addressof(buf)
    ctx = C.c_void_p(base + 120000)
    E = lib.UR_EINVAL
    depth, cmds, idx, cnt, st, oid, keys, res = (C.c_void_p(base + 4096 * k) for k in range(1, 9))
    v, p = lib.fptr(VIEW), lib.fptr(PROJ)
    off = lambda q, k: C.c_void_p(q.value + k)  # noqa: E731
    err = lambda: urlib.ur_last_error().decode()  # noqa: E731
    points = (C.c_uint32 * 128)()

    def draws(**kw):
        d = lib.RasterDraws(cmds, 4, None, None, 0, None)
        for k, val in kw.items():
            setattr(d, k, val)
        return d

    def image(ctx_=ctx, v_=v, p_=p, d=None, depth_=depth, oid_=oid, keys_=keys, w=8, h=8, row0=0, rows=8, flags=0, bits=0, st_=st):
        d = draws() if d is None else d
        return urlib.ur_object_id_pass(ctx_, v_, p_, C.byref(d) if d != "null" else None, depth_, oid_, keys_, w, h, row0, rows, flags, bits, st_)

    def pick(ctx_=ctx, v_=v, p_=p, d=None, depth_=depth, w=8, h=8, flags=0, bits=0, pts=points, n=1, res_=res, st_=st):
        d = draws() if d is None else d
        return urlib.ur_object_id_pick(ctx_, v_, p_, C.byref(d) if d != "null" else None, depth_, w, h, flags, bits, pts, n, res_, st_)

    rg = lib.DrawRanges(idx, 2, cmds, cnt)
    # ur_gbuffer_pass' cases, for both calls
    for call, who in ((image, "ur_object_id_pass"), (pick, "ur_object_id_pick")):
        assert call(ctx_=None) == E and call(v_=None) == E and call(p_=None) == E and call(d="null") == E and call(depth_=None) == E
        assert who in err()
        assert call(w=0) == E and call(h=0) == E and call(w=16385) == E and call(h=16385) == E
        assert call(flags=2) == E and "flag" in err()
        assert call(bits=32) == E and "key_triangle_bits" in err()
        assert call(d=draws(command_count=16), bits=28) == E and "fit" in err()      # 16 slots beside 28 triangle bits
        assert call(d=draws(command_count=1 << 24)) == lib.UR_EUNSUPPORTED
        assert call(d=draws(commands=None)) == E and call(d=draws(commands=off(cmds, 8))) == E
        assert call(depth_=off(depth, 2)) == E and call(st_=off(st, 2)) == E and "misaligned" in err()
        assert call(d=draws(visible_idx=idx)) == E and call(d=draws(visible_count=cnt)) == E
        assert call(d=draws(visible_idx=idx, visible_count=cnt, ranges=C.pointer(rg))) == E
        assert call(d=draws(commands=None, ranges=C.pointer(lib.DrawRanges(idx, 0, cmds, cnt)))) == E
        assert call(d=draws(commands=None, ranges=C.pointer(lib.DrawRanges(None, 2, cmds, cnt)))) == E
    # the image pass' own: the targets and the band
    assert image(oid_=None) == E and image(keys_=None) == E and image(oid_=off(oid, 2)) == E and image(keys_=off(keys, 2)) == E and "object_id or keys" in err()
    assert image(rows=0) == E and image(row0=8, rows=1) == E and image(row0=4, rows=5) == E and "rows" in err()
    # object_id and keys (8 x 8 x 4 = 256 bytes each) over depth (256 bytes), the commands (4 x 64 bytes) and each other, from either side
    for name in ("oid_", "keys_"):
        for q in (depth, cmds):
            assert image(**{name: off(q, 252)}) == E and "overlaps" in err() and image(**{name: off(q, -252)}) == E and "overlaps" in err()
    assert image(oid_=off(keys, 252)) == E and image(keys_=off(oid, 252)) == E and image(oid_=keys) == E and "overlaps" in err()
    assert image(oid_=off(cmds, 252), d=draws(commands=None, ranges=C.pointer(rg))) == E and "overlaps" in err()  # (the ranges' commands)
    # the pick's own: the count, the points, the records
    assert pick(n=65) == E and "65" in err() and pick(n=0xFFFFFFFF) == E
    assert pick(pts=None) == E and "points_xy" in err()
    assert pick(res_=None) == E and pick(res_=off(res, 8)) == E and pick(res_=off(res, 4)) == E and "results" in err()
    assert pick(n=2, res_=off(depth, 240)) == E and "overlaps" in err() and pick(n=64, res_=off(depth, -1008)) == E and pick(res_=off(cmds, 240)) == E and "overlaps" in err()
    # nothing to pick is nothing to do, whatever points_xy and results are; the other arguments are still checked
    assert pick(n=0) == lib.UR_OK and pick(n=0, pts=None, res_=None) == lib.UR_OK and pick(n=0, res_=depth) == lib.UR_OK
    assert pick(n=0, ctx_=None) == E and pick(n=0, flags=4) == E
    del buf


class _FakeTensor:
    def __init__(self, dtype, n, at):
        self.dtype, self._n, self._at, self.is_cuda, self.device = dtype, n, at, True, "cuda"

    def is_contiguous(self):
        return True

    def numel(self):
        return self._n

    def element_size(self):
        return 4

    def data_ptr(self):
        return self._at


def test_python_routing():
    """HotPath.object_id_pass and object_id_pick go to their entry points with the arguments in the header's order."""
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
    depth, cmds = t(torch.float32, 64, 0x1000), t(torch.int32, 64, 0x2000)
    oid, keys, stats, res = t(torch.int32, 64, 0x3000), t(torch.int32, 64, 0x4000), t(torch.int32, 6, 0x5000), t(torch.int32, 12, 0x6000)
    dd = hp.raster_draws(cmds, index_base=3)
    got = hp.HotPath.object_id_pass(Self(), dd, VIEW, PROJ, depth, 8, 8, object_id=oid, keys=keys, row0=2, rows=5, flags=1, key_triangle_bits=20, stats=stats)
    assert got == (oid, keys)
    rec = hp.HotPath.object_id_pick(Self(), cmds, VIEW, PROJ, depth, 8, 8, [(1, 2), (8, 0xFFFFFFFF), (1, 2)], results=res, flags=1, key_triangle_bits=20, stats=stats)
    assert rec is res and [name for name, _ in called] == ["ur_object_id_pass", "ur_object_id_pick"]
    a = called[0][1]
    assert a[0].value == 1 and C.cast(a[3], C.POINTER(lib.RasterDraws)).contents.index_base == 3 and a[4].value == 0x1000 and a[5].value == 0x3000 and a[6].value == 0x4000
    assert a[7:13] == (8, 8, 2, 5, 1, 20) and a[13].value == 0x5000
    a = called[1][1]
    assert C.cast(a[3], C.POINTER(lib.RasterDraws)).contents.commands == 0x2000 and a[4].value == 0x1000 and a[5:9] == (8, 8, 1, 20)
    assert [a[9][k] for k in range(6)] == [1, 2, 8, 0xFFFFFFFF, 1, 2] and a[10] == 3 and a[11].value == 0x6000 and a[12].value == 0x5000  # (the call clamps, not Python)
    with pytest.raises(AssertionError):
        hp.HotPath.object_id_pick(Self(), cmds, VIEW, PROJ, depth, 8, 8, [(0, 0)] * 4, results=res)  # room for 3 records
    with pytest.raises(AssertionError):
        hp.HotPath.object_id_pass(Self(), dd, VIEW, PROJ, depth, 8, 8, object_id=t(torch.int32, 63, 0x3000), keys=keys)
