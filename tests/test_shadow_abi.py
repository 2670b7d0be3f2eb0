"""The ShadowMap pass without a GPU: the new symbols (include/ur_raster.h, ur_frame_set_shadow_pass), struct layouts, the flag and
every argument check that returns before a device is touched."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
LLVM = Path("/opt/rocm/lib/llvm/bin")
NEW = ("ur_shadow_map", "ur_raster_reserve", "ur_frame_set_shadow_pass")


def _headers():
    return "".join(re.sub(r"/\*.*?\*/", "", (ROOT / "include" / h).read_text(), flags=re.S) for h in ("ur_raster.h", "ur_frame.h"))


def test_symbols_declared_exported_and_bound(urlib):
    from unclerenderer_amd import lib
    from unclerenderer_amd import hotpath as hp
    text = _headers()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in lib.SIGNATURES and getattr(urlib, name) is not None
    # the raster entry points live in their own header: include/ur_hotpath.h is the table of tests/footprint.py
    hot = (ROOT / "include" / "ur_hotpath.h").read_text()
    assert "ur_shadow_map" not in hot and "ur_raster_reserve" not in hot
    for cls, names in ((hp.HotPath, ("shadow_map", "raster_reserve")), (hp.Frame, ("set_shadow_pass",)), (hp, ("pack_draw_commands", "raster_draws"))):
        for n in names:
            assert callable(getattr(cls, n)), n
    if not (LLVM / "llvm-readelf").exists():
        pytest.skip("llvm tools not found")
    dyn = subprocess.run([str(LLVM / "llvm-readelf"), "--dyn-syms", "--wide", str(lib.library_path())], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert re.search(r"FUNC\s+GLOBAL\s+DEFAULT\s+\d+\s+%s$" % name, dyn, re.M), name


def test_struct_layouts_match_the_headers():
    from unclerenderer_amd import lib
    text = (ROOT / "include" / "ur_raster.h").read_text() + (ROOT / "include" / "ur_frame.h").read_text()

    def fields(name):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        return [re.findall(r"(\w+)\s*(?:\[\d+\])?\s*$", part.strip())[0] for decl in body.split(";") if decl.strip() for part in decl.split(",")]

    assert fields("ur_raster_draws") == [n for n, _ in lib.RasterDraws._fields_]
    assert fields("ur_frame_shadow_pass") == [n for n, _ in lib.FrameShadowPass._fields_]
    D = lib.RasterDraws
    assert [(getattr(D, n).offset, getattr(D, n).size) for n, _ in D._fields_] == [(0, 8), (8, 4), (16, 8), (24, 8), (32, 4), (40, 8)]
    assert C.sizeof(D) == 48
    S = lib.FrameShadowPass
    assert C.sizeof(S) == 64 and S.shadow_map.offset == 48 and S.stats4.offset == 56
    assert lib.UR_RASTER_MAX_TARGET == int(re.search(r"#define UR_RASTER_MAX_TARGET (\d+)u", text).group(1)) == 16384
    assert lib.UR_RASTER_INDEX_FORMAT_R32_UINT == int(re.search(r"#define UR_RASTER_INDEX_FORMAT_R32_UINT (\d+)u", text).group(1)) == 42


def test_flag_is_new():
    from unclerenderer_amd import lib
    assert lib.UR_FRAME_SHADOW_PASS == 0x8000000
    others = [getattr(lib, n) for n in dir(lib) if n.startswith("UR_FRAME_") and n not in ("UR_FRAME_SHADOW_PASS", "UR_FRAME_DEFAULT")]
    assert len(others) >= 27 and all(o & lib.UR_FRAME_SHADOW_PASS == 0 for o in others)
    assert lib.UR_FRAME_DEFAULT & lib.UR_FRAME_SHADOW_PASS == 0
    header = (ROOT / "include" / "ur_frame.h").read_text()
    defined = {m.group(1): int(m.group(2), 16) for m in re.finditer(r"#define (UR_FRAME_\w+) 0x([0-9a-fA-F]+)u", header)}
    assert defined["UR_FRAME_SHADOW_PASS"] == 0x8000000 and len(set(defined.values())) == len(defined)
    for k, v in defined.items():
        assert getattr(lib, k) == v, k


ORTHO = np.array([0.5, 0, 0, 0, 0, 0.25, 0, 0, 0, 0, 0.125, 0, 0.1, 0.2, 0.3, 1], np.float32)


def _stand_ins():
    buf = (C.c_uint64 * 8192)()
    base = C.addressof(buf)
    return buf, base, C.c_void_p(base + 60000)  # a context that is never dereferenced: every check below returns before it is used


def test_shadow_map_argument_checks(urlib):
    from unclerenderer_amd import lib
    buf, base, ctx = _stand_ins()
    E, U = lib.UR_EINVAL, lib.UR_EUNSUPPORTED
    f = urlib.ur_shadow_map
    m, cmds, idx, cnt, st = (C.c_void_p(base + 4096 * k) for k in range(1, 6))
    lvp = lib.fptr(ORTHO)

    def draws(**kw):
        d = lib.RasterDraws(cmds, 4, None, None, 0, None)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    ok = draws()
    assert f(None, lvp, C.byref(ok), m, 64, 64, st) == E and "null" in urlib.ur_last_error().decode()
    assert f(ctx, None, C.byref(ok), m, 64, 64, st) == E
    assert f(ctx, lvp, None, m, 64, 64, st) == E
    assert f(ctx, lvp, C.byref(ok), None, 64, 64, st) == E
    assert f(ctx, lvp, C.byref(draws(commands=None)), m, 64, 64, st) == E          # slots without a buffer
    for w, h in ((0, 64), (64, 0), (16385, 64), (64, 16385)):
        assert f(ctx, lvp, C.byref(ok), m, w, h, st) == E, (w, h)
    assert "ur_shadow_map" in urlib.ur_last_error().decode()
    assert f(ctx, lvp, C.byref(draws(visible_idx=idx)), m, 64, 64, st) == E       # a list without its count
    assert f(ctx, lvp, C.byref(draws(visible_count=cnt)), m, 64, 64, st) == E     # a count without its list
    rg = lib.DrawRanges(idx, 2, cmds, cnt)
    both = draws(visible_idx=idx, visible_count=cnt, ranges=C.pointer(rg))
    assert f(ctx, lvp, C.byref(both), m, 64, 64, st) == E                          # both selections
    for hole in ("offsets", "commands", "counts"):
        bad = lib.DrawRanges(idx, 2, cmds, cnt)
        setattr(bad, hole, None)
        assert f(ctx, lvp, C.byref(draws(ranges=C.pointer(bad))), m, 64, 64, st) == E, hole
    assert f(ctx, lvp, C.byref(draws(ranges=C.pointer(lib.DrawRanges(idx, 0, cmds, cnt)))), m, 64, 64, st) == E
    # misaligned buffers: commands 16 bytes, the others 4
    off = lambda p, k: C.c_void_p(p.value + k)  # noqa: E731
    assert f(ctx, lvp, C.byref(draws(commands=off(cmds, 8))), m, 64, 64, st) == E
    assert f(ctx, lvp, C.byref(ok), off(m, 2), 64, 64, st) == E
    assert f(ctx, lvp, C.byref(ok), m, 64, 64, off(st, 1)) == E
    assert f(ctx, lvp, C.byref(draws(visible_idx=off(idx, 2), visible_count=cnt)), m, 64, 64, st) == E
    assert f(ctx, lvp, C.byref(draws(visible_idx=idx, visible_count=off(cnt, 2))), m, 64, 64, st) == E
    assert f(ctx, lvp, C.byref(draws(ranges=C.pointer(lib.DrawRanges(idx, 2, off(cmds, 4), cnt)))), m, 64, 64, st) == E
    assert "misaligned" in urlib.ur_last_error().decode()
    # a perspective light: the fourth column is not exactly (0, 0, 0, 1)
    for at, v in ((3, 1e-30), (7, -0.5), (11, 1.0), (15, 0.99999994), (15, float("nan"))):
        p = ORTHO.copy()
        p[at] = v
        assert f(ctx, lib.fptr(p), C.byref(ok), m, 64, 64, st) == U, (at, v)
    assert "orthographic" in urlib.ur_last_error().decode()
    p = ORTHO.copy()
    p[3] = -0.0  # -0 is 0
    assert f(ctx, lib.fptr(p), C.byref(draws(commands=off(cmds, 8))), m, 64, 64, st) == E  # (argument errors come first)
    assert urlib.ur_raster_reserve(None, 16) == E
    del buf


def test_frame_shadow_pass_argument_checks(urlib):
    """ur_frame_set_shadow_pass and ur_frame_render's checks of the flag on a frame made over a stand-in context."""
    from unclerenderer_amd import lib
    buf, base, ctx = _stand_ins()
    E = lib.UR_EINVAL
    m, cmds, idx, cnt, st, other = (C.c_void_p(base + 4096 * k) for k in range(1, 7))
    assert urlib.ur_frame_set_shadow_pass(None, None) == E
    f = C.c_void_p(urlib.ur_frame_create(ctx, None, 2, 0, 1))
    assert f.value

    def sp(shadow_map=m, stats=st, **kw):
        d = lib.RasterDraws(cmds, 4, None, None, 0, None)
        for k, v in kw.items():
            setattr(d, k, v)
        return lib.FrameShadowPass(d, shadow_map, stats)

    assert urlib.ur_frame_set_shadow_pass(f, C.byref(sp(shadow_map=None))) == E
    assert urlib.ur_frame_set_shadow_pass(f, C.byref(sp(visible_idx=idx))) == E
    rg = lib.DrawRanges(idx, 2, cmds, cnt)
    assert urlib.ur_frame_set_shadow_pass(f, C.byref(sp(visible_idx=idx, visible_count=cnt, ranges=C.pointer(rg)))) == E
    assert urlib.ur_frame_set_shadow_pass(f, C.byref(sp(ranges=C.pointer(lib.DrawRanges(idx, 0, cmds, cnt))))) == E
    assert urlib.ur_frame_set_shadow_pass(f, C.byref(sp(commands=None))) == E
    assert urlib.ur_frame_set_shadow_pass(f, C.byref(sp(commands=C.c_void_p(cmds.value + 4)))) == E
    assert urlib.ur_frame_set_shadow_pass(f, C.byref(sp(shadow_map=C.c_void_p(m.value + 1)))) == E

    res = lib.FrameResources()
    res.width, res.height, res.row0, res.rows = 64, 32, 0, 32
    res.tables.shadow_map = other
    consts = (C.c_uint32 * lib.UR_CULL_CONSTANT_DWORDS)()
    scene, sky = lib.SceneConstants(), lib.SkyConstants()
    flags = lib.UR_FRAME_DEFAULT | lib.UR_FRAME_SHADOW_PASS
    render = lambda fl: urlib.ur_frame_render(f, C.byref(res), consts, C.byref(scene), C.byref(sky), fl)  # noqa: E731
    assert render(flags) == E and "ur_frame_set_shadow_pass" in urlib.ur_last_error().decode()   # the flag without a pass
    assert urlib.ur_frame_set_shadow_pass(f, C.byref(sp(ranges=C.pointer(rg), commands=None))) == lib.UR_OK
    assert urlib.ur_frame_set_shadow_pass(f, C.byref(sp(visible_idx=idx, visible_count=cnt))) == lib.UR_OK
    assert render(flags) == E and "tables.shadow_map" in urlib.ur_last_error().decode()         # Lighting would read another map
    assert urlib.ur_frame_set_shadow_pass(f, None) == lib.UR_OK                                  # cleared
    assert render(flags) == E and "ur_frame_set_shadow_pass" in urlib.ur_last_error().decode()
    urlib.ur_frame_destroy(f)
    del buf
