"""GpuDebugPrint without a GPU: the new symbols, struct layouts, the flag, every argument check of the C-ABI and of the frame, the
built-in font's table, and the gfx950 code of the three kernels (no scratch, no spills)."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests.code_objects import LLVM, code_objects, kernel_metadata

ROOT = Path(__file__).resolve().parent.parent
NEW = ("ur_debug_print_buffer_bytes", "ur_debug_print_reset", "ur_debug_print_stats", "ur_debug_print_text", "ur_debug_print_draw",
       "ur_host_debug_font", "ur_frame_set_debug_print")


def test_symbols_and_layouts(urlib):
    from unclerenderer_amd import dist, hostmath, lib
    from unclerenderer_amd.hotpath import Frame, HotPath
    text = "".join(re.sub(r"/\*.*?\*/", "", (ROOT / "include" / h).read_text(), flags=re.S) for h in ("ur_hotpath.h", "ur_frame.h", "ur_host.h"))
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in lib.SIGNATURES and getattr(urlib, name) is not None
    assert C.sizeof(lib.DebugGlyph) == 40 and lib.DebugGlyph.Advance.offset == 32
    assert C.sizeof(lib.DebugPrintConstants) == 16 and lib.DebugPrintConstants.FirstChar.offset == 8
    assert "} ur_debug_glyph;" in text and "} ur_debug_print_constants;" in text
    assert urlib.ur_debug_print_buffer_bytes() == 4 + 4096 * 16
    assert lib.UR_DEBUG_PRINT_MAX_ENTRIES == int(re.search(r"#define UR_DEBUG_PRINT_MAX_ENTRIES (\d+)u", text).group(1)) == 4096
    for cls, names in ((HotPath, ("debug_print_reset", "debug_print_stats", "debug_print_text", "debug_print_draw", "debug_print_buffer_bytes")),
                       (Frame, ("set_debug_print",)), (hostmath, ("debug_font",)), (dist, ("allreduce_cull_stats",))):
        for n in names:
            assert callable(getattr(cls, n)), n
    if (LLVM / "llvm-readelf").exists():
        dyn = subprocess.run([str(LLVM / "llvm-readelf"), "--dyn-syms", "--wide", str(lib.library_path())], capture_output=True, text=True, check=True).stdout
        for name in NEW:
            assert re.search(r"FUNC\s+GLOBAL\s+DEFAULT\s+\d+\s+%s$" % name, dyn, re.M), name


def test_flag_does_not_collide():
    from unclerenderer_amd import lib
    assert lib.UR_FRAME_DEBUG_PRINT == 0x4000000
    old = [getattr(lib, n) for n in dir(lib) if n.startswith("UR_FRAME_") and n not in ("UR_FRAME_DEBUG_PRINT", "UR_FRAME_DEFAULT")]
    assert len(old) >= 25 and all(lib.UR_FRAME_DEBUG_PRINT & o == 0 for o in old)
    header = (ROOT / "include" / "ur_frame.h").read_text()
    defined = {m.group(1): int(m.group(2), 16) for m in re.finditer(r"#define (UR_FRAME_\w+) 0x([0-9a-fA-F]+)u", header)}
    assert defined["UR_FRAME_DEBUG_PRINT"] == 0x4000000 and len(set(defined.values())) == len(defined)
    assert lib.UR_FRAME_DEFAULT & lib.UR_FRAME_DEBUG_PRINT == 0


def test_argument_errors_return_einval(urlib):
    """Every check returns before the context or a device pointer is used (a stand-in context that is never dereferenced)."""
    from unclerenderer_amd import lib
    mem = (C.c_uint64 * 8192)()
    base = C.addressof(mem)
    ctx, p, q, r, s = (C.c_void_p(base + k * 8192) for k in (6, 0, 1, 2, 3))
    E = lib.UR_EINVAL
    k = lib.DebugPrintConstants((C.c_float * 2)(16, 16), 32, 96)
    assert urlib.ur_debug_print_reset(None, p, None) == E and urlib.ur_debug_print_reset(ctx, None, q) == E
    assert "ur_debug_print_reset" in urlib.ur_last_error().decode()
    assert urlib.ur_debug_print_stats(None, p, q) == E and urlib.ur_debug_print_stats(ctx, None, q) == E and urlib.ur_debug_print_stats(ctx, p, None) == E
    assert urlib.ur_debug_print_text(None, p, 0, 0, 0, b"A", 1) == E and urlib.ur_debug_print_text(ctx, None, 0, 0, 0, b"A", 1) == E
    assert urlib.ur_debug_print_text(ctx, p, 0, 0, 0, None, 1) == E
    assert urlib.ur_debug_print_text(ctx, p, 0, 0, 0, None, 0) == lib.UR_OK      # nothing to print launches nothing
    assert urlib.ur_debug_print_text(ctx, p, 0, 0, 0, b"\0AB", 3) == lib.UR_OK   # a string that starts with a zero code neither
    f = urlib.ur_debug_print_draw
    ok = dict(ctx=ctx, k=C.byref(k), glyphs=p, n=96, atlas=q, aw=64, ah=64, buf=r, ldr=s, w=16, h=16, row0=0, rows=16)

    def draw(**kw):
        a = dict(ok, **kw)
        return f(a["ctx"], a["k"], a["glyphs"], a["n"], a["atlas"], a["aw"], a["ah"], a["buf"], a["ldr"], a["w"], a["h"], a["row0"], a["rows"])

    for bad in (dict(ctx=None), dict(k=None), dict(glyphs=None), dict(atlas=None), dict(buf=None), dict(ldr=None), dict(n=0), dict(aw=0), dict(ah=0),
                dict(aw=1 << 20), dict(row0=8, rows=9), dict(row0=17, rows=0), dict(w=0), dict(h=0, rows=0), dict(w=32), dict(h=32)):
        assert draw(**bad) == E, bad
        assert "ur_debug_print_draw" in urlib.ur_last_error().decode()
    assert draw(rows=0) == lib.UR_OK and draw(row0=16, rows=0) == lib.UR_OK  # an empty band launches nothing
    # the font
    info = (C.c_uint32 * 4)()
    assert urlib.ur_host_debug_font(None, 0, None, 0, None) == E
    assert urlib.ur_host_debug_font(None, 0, None, 0, info) == lib.UR_OK and list(info) == [64, 64, 32, 64]
    assert urlib.ur_host_debug_font(p, 4096, None, 96, info) == E and urlib.ur_host_debug_font(None, 4096, q, 96, info) == E
    assert urlib.ur_host_debug_font(p, 4095, q, 96, info) == E and urlib.ur_host_debug_font(p, 4096, q, 95, info) == E


def test_frame_argument_checks(urlib):
    from unclerenderer_amd import lib
    mem = (C.c_uint64 * 8192)()
    base = C.addressof(mem)
    ctx = C.c_void_p(base + 60000)
    E = lib.UR_EINVAL
    assert urlib.ur_frame_set_debug_print(None, None) == E
    f = C.c_void_p(urlib.ur_frame_create(ctx, None, 2, 0, 1))
    assert f
    try:
        good = dict(buffer=base, glyphs=base + 4096, glyph_count=96, atlas=base + 8192, atlas_w=64, atlas_h=64, first_char=32, char_count=64)
        for hole in ("buffer", "glyphs", "glyph_count", "atlas", "atlas_w", "atlas_h"):
            dp = lib.FrameDebugPrint(**dict(good, **{hole: 0 if "_" in hole else None}))
            assert urlib.ur_frame_set_debug_print(f, C.byref(dp)) == E, hole
        res = lib.FrameResources()
        res.width, res.height, res.row0, res.rows = 16, 16, 0, 16
        res.tonemap_band, res.cull_stats = base + 16384, base + 20000
        cc = (C.c_uint32 * lib.UR_CULL_CONSTANT_DWORDS)()
        scene, sky = lib.SceneConstants(), lib.SkyConstants()
        DP, TM = lib.UR_FRAME_DEBUG_PRINT, lib.UR_FRAME_TONEMAP

        def render(flags):
            return urlib.ur_frame_render(f, C.byref(res), cc, C.byref(scene), C.byref(sky), flags)

        assert render(TM | DP) == E and "ur_frame_set_debug_print" in urlib.ur_last_error().decode()  # no buffer / font yet
        assert urlib.ur_frame_set_debug_print(f, C.byref(lib.FrameDebugPrint(**good))) == lib.UR_OK
        assert render(DP) == E                                     # without TONEMAP
        res.tonemap_band = None
        assert render(TM | DP) == E                                # without a tonemap_band
        res.tonemap_band, res.cull_stats = base + 16384, None
        assert render(TM | DP) == E and "cull_stats" in urlib.ur_last_error().decode()
        res.cull_stats = base + 20000
        assert urlib.ur_frame_set_debug_print(f, None) == lib.UR_OK  # NULL clears
        assert render(TM | DP) == E
    finally:
        urlib.ur_frame_destroy(f)


def test_builtin_font_table_is_well_formed(urlib):
    from unclerenderer_amd import hostmath
    atlas, glyphs, first, count = hostmath.debug_font()
    assert (first, count) == (32, 64) and atlas.shape == (64, 64) and atlas.dtype == np.uint8 and glyphs.shape == (96, 10)
    assert set(np.unique(atlas)) == {0, 255}
    assert not glyphs[:first].any()
    cells = set()
    for code in range(first, first + count):
        u0, v0, u1, v1, sw, sh, ox, oy, adv, pad = (float(v) for v in glyphs[code])
        assert 0.0 <= u0 < u1 <= 1.0 and 0.0 <= v0 < v1 <= 1.0, code       # UVs inside the atlas
        assert adv == 8.0 and pad == 0.0 and (sw, sh) == (8.0, 8.0) and (ox, oy) == (0.0, -7.0), code
        x0, y0, x1, y1 = u0 * 64, v0 * 64, u1 * 64, v1 * 64
        assert (x0, y0, x1, y1) == (int(x0), int(y0), int(x0) + 8, int(y0) + 8)  # one whole 8 x 8 cell, texel-aligned
        cells.add((int(x0), int(y0)))
        cell = atlas[int(y0):int(y1), int(x0):int(x1)]
        assert not cell[7].any() and not cell[:, 0].any() and not cell[:, 6:].any()  # 5 x 7 dots in columns 1..5, rows 0..6
        assert cell.any() == (code != 32), code                                       # only the space is blank
    assert len(cells) == 64
    shapes = {atlas[y:y + 8, x:x + 8].tobytes() for x, y in cells}
    assert len(shapes) == 64  # every glyph is a shape of its own ('0' and 'O', '1' and 'I' included)


def test_kernels_use_no_scratch(urlib, tmp_path, record_property):
    """The gfx950 code of the stats, text and draw kernels: no scratch, no VGPR or SGPR spills. Register counts are recorded."""
    from unclerenderer_amd import lib
    if not (LLVM / "llvm-readelf").exists():
        pytest.skip("llvm tools not found")
    meta = {}
    for co in code_objects(lib.library_path(), tmp_path):
        meta.update({k: v for k, v in kernel_metadata(co).items() if "debug_print_" in k})
    for want in ("debug_print_stats_kernel", "debug_print_text_kernel", "debug_print_draw_kernel"):
        hits = [k for k in meta if want in k]
        assert len(hits) == 1, (want, sorted(meta))
        m = meta[hits[0]]
        record_property(want + ".vgpr_count", m["vgpr_count"])
        print(want, m)
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (want, m)
