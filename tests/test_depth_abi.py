"""The DepthPrepass pass without a GPU: the new symbols (ur_depth_prepass in include/ur_raster.h, ur_frame_set_depth_pass), struct
layouts, the flags and every argument check that returns before a device is touched."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
LLVM = Path("/opt/rocm/lib/llvm/bin")
NEW = ("ur_depth_prepass", "ur_frame_set_depth_pass")

VIEW = np.eye(4, dtype=np.float32).reshape(-1)
PROJ = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 0.125, 0], np.float32)


def test_symbols_declared_exported_and_bound(urlib):
    from unclerenderer_amd import lib
    from unclerenderer_amd import hotpath as hp
    raster = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "ur_raster.h").read_text(), flags=re.S)
    frame = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "ur_frame.h").read_text(), flags=re.S)
    assert re.search(r"\bur_depth_prepass\s*\(", raster) and re.search(r"\bur_frame_set_depth_pass\s*\(", frame)
    assert "ur_depth_prepass" not in (ROOT / "include" / "ur_hotpath.h").read_text()
    for name in NEW:
        assert name in lib.SIGNATURES and getattr(urlib, name) is not None
    assert callable(hp.HotPath.depth_prepass) and callable(hp.Frame.set_depth_pass)
    if not (LLVM / "llvm-readelf").exists():
        pytest.skip("llvm tools not found")
    dyn = subprocess.run([str(LLVM / "llvm-readelf"), "--dyn-syms", "--wide", str(lib.library_path())], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert re.search(r"FUNC\s+GLOBAL\s+DEFAULT\s+\d+\s+%s$" % name, dyn, re.M), name


def test_struct_layout_and_constants_match_the_headers():
    from unclerenderer_amd import lib
    raster, frame = (ROOT / "include" / "ur_raster.h").read_text(), (ROOT / "include" / "ur_frame.h").read_text()
    body = re.search(r"typedef struct ur_frame_depth_pass \{(.*?)\} ur_frame_depth_pass;", frame, re.S).group(1)
    names = [re.findall(r"(\w+)\s*$", d.strip())[0] for d in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";") if d.strip()]
    S = lib.FrameDepthPass
    assert names == [n for n, _ in S._fields_] == ["draws", "depth", "stats6", "flags"]
    assert (S.depth.offset, S.stats6.offset, S.flags.offset, C.sizeof(S)) == (48, 56, 64, 72)
    assert lib.UR_DEPTH_QUANTIZE_D24 == int(re.search(r"#define UR_DEPTH_QUANTIZE_D24 0x([0-9a-fA-F]+)u", raster).group(1), 16) == 1
    assert lib.UR_DEPTH_GUARD_BAND == int(re.search(r"#define UR_DEPTH_GUARD_BAND (\d+)u", raster).group(1)) == 2 ** 21
    assert lib.UR_FRAME_DEPTH_PASS == 0x10000000
    defined = {m.group(1): int(m.group(2), 16) for m in re.finditer(r"#define (UR_FRAME_\w+) 0x([0-9a-fA-F]+)u", frame)}
    assert defined["UR_FRAME_DEPTH_PASS"] == 0x10000000 and len(set(defined.values())) == len(defined)
    others = [v for k, v in defined.items() if k != "UR_FRAME_DEPTH_PASS"]
    assert all(v & 0x10000000 == 0 for v in others) and lib.UR_FRAME_DEFAULT & lib.UR_FRAME_DEPTH_PASS == 0
    for k, v in defined.items():
        assert getattr(lib, k) == v, k


def _stand_ins():
    buf = (C.c_uint64 * 8192)()
    base = C.addressof(buf)
    return buf, base, C.c_void_p(base + 60000)  # a context that is never dereferenced: every check below returns before it is used


def test_depth_prepass_argument_checks(urlib):
    from unclerenderer_amd import lib
    buf, base, ctx = _stand_ins()
    E = lib.UR_EINVAL
    f = urlib.ur_depth_prepass
    m, cmds, idx, cnt, st = (C.c_void_p(base + 4096 * k) for k in range(1, 6))
    v, p = lib.fptr(VIEW), lib.fptr(PROJ)

    def draws(**kw):
        d = lib.RasterDraws(cmds, 4, None, None, 0, None)
        for k, val in kw.items():
            setattr(d, k, val)
        return d

    ok = draws()
    assert f(None, v, p, C.byref(ok), m, 64, 64, 0, st) == E and "null" in urlib.ur_last_error().decode()
    assert f(ctx, None, p, C.byref(ok), m, 64, 64, 0, st) == E
    assert f(ctx, v, None, C.byref(ok), m, 64, 64, 0, st) == E
    assert f(ctx, v, p, None, m, 64, 64, 0, st) == E
    assert f(ctx, v, p, C.byref(ok), None, 64, 64, 0, st) == E
    assert f(ctx, v, p, C.byref(draws(commands=None)), m, 64, 64, 0, st) == E          # slots without a buffer
    for w, h in ((0, 64), (64, 0), (16385, 64), (64, 16385)):
        assert f(ctx, v, p, C.byref(ok), m, w, h, 0, st) == E, (w, h)
    assert "ur_depth_prepass" in urlib.ur_last_error().decode()
    assert f(ctx, v, p, C.byref(draws(visible_idx=idx)), m, 64, 64, 0, st) == E       # a list without its count
    assert f(ctx, v, p, C.byref(draws(visible_count=cnt)), m, 64, 64, 0, st) == E     # a count without its list
    rg = lib.DrawRanges(idx, 2, cmds, cnt)
    both = draws(visible_idx=idx, visible_count=cnt, ranges=C.pointer(rg))
    assert f(ctx, v, p, C.byref(both), m, 64, 64, 0, st) == E                          # both selections
    for hole in ("offsets", "commands", "counts"):
        bad = lib.DrawRanges(idx, 2, cmds, cnt)
        setattr(bad, hole, None)
        assert f(ctx, v, p, C.byref(draws(ranges=C.pointer(bad))), m, 64, 64, 0, st) == E, hole
    assert f(ctx, v, p, C.byref(draws(ranges=C.pointer(lib.DrawRanges(idx, 0, cmds, cnt)))), m, 64, 64, 0, st) == E
    off = lambda q, k: C.c_void_p(q.value + k)  # noqa: E731
    assert f(ctx, v, p, C.byref(draws(commands=off(cmds, 8))), m, 64, 64, 0, st) == E
    assert f(ctx, v, p, C.byref(ok), off(m, 2), 64, 64, 0, st) == E
    assert f(ctx, v, p, C.byref(ok), m, 64, 64, 0, off(st, 1)) == E
    assert f(ctx, v, p, C.byref(draws(visible_idx=off(idx, 2), visible_count=cnt)), m, 64, 64, 0, st) == E
    assert f(ctx, v, p, C.byref(draws(visible_idx=idx, visible_count=off(cnt, 2))), m, 64, 64, 0, st) == E
    assert f(ctx, v, p, C.byref(draws(ranges=C.pointer(lib.DrawRanges(idx, 2, off(cmds, 4), cnt)))), m, 64, 64, 0, st) == E
    assert "misaligned" in urlib.ur_last_error().decode()
    # flag bits: only UR_DEPTH_QUANTIZE_D24 is known
    for flags in (0x2, 0x3, 0x80000000, 0xFFFFFFFE):
        assert f(ctx, v, p, C.byref(ok), m, 64, 64, flags, st) == E, hex(flags)
        assert "flag" in urlib.ur_last_error().decode()
    del buf


def test_frame_depth_pass_argument_checks(urlib):
    """ur_frame_set_depth_pass and ur_frame_render's checks of the flag on a frame made over a stand-in context."""
    from unclerenderer_amd import lib
    buf, base, ctx = _stand_ins()
    E = lib.UR_EINVAL
    m, cmds, idx, cnt, st, other = (C.c_void_p(base + 4096 * k) for k in range(1, 7))
    assert urlib.ur_frame_set_depth_pass(None, None) == E
    f = C.c_void_p(urlib.ur_frame_create(ctx, None, 2, 0, 1))
    assert f.value

    def dp(depth=m, stats=st, flags=0, **kw):
        d = lib.RasterDraws(cmds, 4, None, None, 0, None)
        for k, v in kw.items():
            setattr(d, k, v)
        return lib.FrameDepthPass(d, depth, stats, flags)

    set_pass = urlib.ur_frame_set_depth_pass
    assert set_pass(f, C.byref(dp(depth=None))) == E
    assert set_pass(f, C.byref(dp(visible_idx=idx))) == E
    rg = lib.DrawRanges(idx, 2, cmds, cnt)
    assert set_pass(f, C.byref(dp(visible_idx=idx, visible_count=cnt, ranges=C.pointer(rg)))) == E
    assert set_pass(f, C.byref(dp(ranges=C.pointer(lib.DrawRanges(idx, 0, cmds, cnt))))) == E
    assert set_pass(f, C.byref(dp(commands=None))) == E
    assert set_pass(f, C.byref(dp(commands=C.c_void_p(cmds.value + 4)))) == E
    assert set_pass(f, C.byref(dp(depth=C.c_void_p(m.value + 1)))) == E
    assert set_pass(f, C.byref(dp(stats=C.c_void_p(st.value + 2)))) == E
    assert set_pass(f, C.byref(dp(flags=2))) == E and "flag" in urlib.ur_last_error().decode()

    res = lib.FrameResources()
    res.width, res.height, res.row0, res.rows = 64, 32, 0, 32
    res.depth_full = other
    consts = (C.c_uint32 * lib.UR_CULL_CONSTANT_DWORDS)()
    scene, sky = lib.SceneConstants(), lib.SkyConstants()
    flags = lib.UR_FRAME_DEFAULT | lib.UR_FRAME_DEPTH_PASS
    render = lambda fl: urlib.ur_frame_render(f, C.byref(res), consts, C.byref(scene), C.byref(sky), fl)  # noqa: E731
    assert render(flags) == E and "ur_frame_set_depth_pass" in urlib.ur_last_error().decode()   # the flag without a pass
    assert set_pass(f, C.byref(dp(ranges=C.pointer(rg), commands=None))) == lib.UR_OK
    assert set_pass(f, C.byref(dp(visible_idx=idx, visible_count=cnt, flags=lib.UR_DEPTH_QUANTIZE_D24))) == lib.UR_OK
    assert render(flags) == E and "depth_full" in urlib.ur_last_error().decode()                 # Build HZB would read another buffer
    assert set_pass(f, None) == lib.UR_OK                                                        # cleared
    assert render(flags) == E and "ur_frame_set_depth_pass" in urlib.ur_last_error().decode()
    urlib.ur_frame_destroy(f)
    del buf
