"""The GBuffer pass without a GPU: the new symbols (ur_gbuffer_pass in include/ur_raster.h, ur_host_srgb_encode_table,
ur_frame_set_gbuffer_pass), struct layouts, the flag and every argument check that returns before a device is touched."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
LLVM = Path("/opt/rocm/lib/llvm/bin")
NEW = ("ur_gbuffer_pass", "ur_gbuffer_pass_parts", "ur_host_srgb_encode_table", "ur_frame_set_gbuffer_pass")

VIEW = np.eye(4, dtype=np.float32).reshape(-1)
PROJ = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 0.125, 0], np.float32)


def _strip(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_symbols_declared_exported_and_bound(urlib):
    from unclerenderer_amd import hostmath, lib
    from unclerenderer_amd import hotpath as hp
    raster, frame, host = (_strip((ROOT / "include" / n).read_text()) for n in ("ur_raster.h", "ur_frame.h", "ur_host.h"))
    assert re.search(r"\bur_gbuffer_pass\s*\(", raster) and re.search(r"\bur_gbuffer_pass_parts\s*\(", raster) and re.search(r"\bur_frame_set_gbuffer_pass\s*\(", frame)
    assert re.search(r"\bur_host_srgb_encode_table\s*\(", host)
    for name in NEW:
        assert name in lib.SIGNATURES and getattr(urlib, name) is not None
    assert callable(hp.HotPath.gbuffer_pass) and callable(hp.Frame.set_gbuffer_pass) and callable(hostmath.srgb_encode_table)
    if not (LLVM / "llvm-readelf").exists():
        pytest.skip("llvm tools not found")
    dyn = subprocess.run([str(LLVM / "llvm-readelf"), "--dyn-syms", "--wide", str(lib.library_path())], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert re.search(r"FUNC\s+GLOBAL\s+DEFAULT\s+\d+\s+%s$" % name, dyn, re.M), name


def _names(header, struct):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, re.S).group(1)
    return [re.findall(r"(\w+)\s*$", d.strip())[0] for d in _strip(body).split(";") if d.strip()]


def test_struct_layout_and_constants_match_the_headers():
    from unclerenderer_amd import lib
    raster, frame = (ROOT / "include" / "ur_raster.h").read_text(), (ROOT / "include" / "ur_frame.h").read_text()
    T, P = lib.GBufferTargets, lib.FrameGBufferPass
    assert _names(raster, "ur_gbuffer_targets") == [n for n, _ in T._fields_] == ["gbuf_a", "gbuf_b", "gbuf_c", "hdr", "object_id", "keys"]
    assert [getattr(T, n).offset for n, _ in T._fields_] == [0, 8, 16, 24, 32, 40] and C.sizeof(T) == 48
    assert _names(frame, "ur_frame_gbuffer_pass") == [n for n, _ in P._fields_] == ["draws", "targets", "stats6", "flags", "key_triangle_bits"]
    assert (P.targets.offset, P.stats6.offset, P.flags.offset, P.key_triangle_bits.offset, C.sizeof(P)) == (48, 96, 104, 108, 112)
    defined = {m.group(1): int(m.group(2), 16) for m in re.finditer(r"#define (UR_FRAME_\w+) 0x([0-9a-fA-F]+)u", frame)}
    assert lib.UR_FRAME_GBUFFER_PASS == defined["UR_FRAME_GBUFFER_PASS"] == 0x20000000 and len(set(defined.values())) == len(defined)
    assert all(v & 0x20000000 == 0 for k, v in defined.items() if k != "UR_FRAME_GBUFFER_PASS")
    assert lib.UR_FRAME_DEFAULT & lib.UR_FRAME_GBUFFER_PASS == 0
    for k, v in defined.items():
        assert getattr(lib, k) == v, k


def _stand_ins():
    buf = (C.c_uint64 * 16384)()
    base = C.addressof(buf)
    return buf, base, C.c_void_p(base + 120000)  # a context that is never dereferenced: every check below returns before it is used


def test_gbuffer_pass_argument_checks(urlib):
    from unclerenderer_amd import lib
    buf, base, ctx = _stand_ins()
    E = lib.UR_EINVAL
    f = urlib.ur_gbuffer_pass
    depth, cmds, idx, cnt, st, a, b, c, hdr, oid, keys = (C.c_void_p(base + 4096 * k) for k in range(1, 12))
    v, p = lib.fptr(VIEW), lib.fptr(PROJ)
    header = (ROOT / "include" / "ur_raster.h").read_text()
    off = lambda q, k: C.c_void_p(q.value + k)  # noqa: E731

    def draws(**kw):
        d = lib.RasterDraws(cmds, 4, None, None, 0, None)
        for k, val in kw.items():
            setattr(d, k, val)
        return d

    def targets(**kw):
        t = lib.GBufferTargets(a, b, c, hdr, oid, keys)
        for k, val in kw.items():
            setattr(t, k, val)
        return t

    ok, tg = draws(), targets()
    call = lambda ctx_=ctx, v_=v, p_=p, d=ok, depth_=depth, t=tg, w=64, h=64, row0=0, rows=64, flags=0, bits=0, st_=st: \
        f(ctx_, v_, p_, C.byref(d) if d is not None else None, depth_, C.byref(t) if t is not None else None, w, h, row0, rows, flags, bits, st_)  # noqa: E731
    # ur_depth_prepass' cases
    assert call(ctx_=None) == E and "null" in urlib.ur_last_error().decode()
    assert call(v_=None) == E and call(p_=None) == E and call(d=None) == E and call(depth_=None) == E
    assert call(d=draws(commands=None)) == E
    for w, h in ((0, 64), (64, 0), (16385, 64), (64, 16385)):
        assert call(w=w, h=h, rows=1) == E, (w, h)
    assert "ur_gbuffer_pass" in urlib.ur_last_error().decode()
    assert call(d=draws(visible_idx=idx)) == E and call(d=draws(visible_count=cnt)) == E
    rg = lib.DrawRanges(idx, 2, cmds, cnt)
    assert call(d=draws(visible_idx=idx, visible_count=cnt, ranges=C.pointer(rg))) == E
    assert call(d=draws(ranges=C.pointer(lib.DrawRanges(idx, 0, cmds, cnt)))) == E
    assert call(d=draws(commands=off(cmds, 8))) == E and call(depth_=off(depth, 2)) == E and call(st_=off(st, 1)) == E
    for flags in (0x2, 0x80000000):
        assert call(flags=flags) == E and "flag" in urlib.ur_last_error().decode()
    # the pass' own
    assert call(t=None) == E
    for name in ("gbuf_a", "gbuf_b", "gbuf_c", "hdr", "keys"):
        assert call(t=targets(**{name: None})) == E and "target" in urlib.ur_last_error().decode(), name
    for name, by in (("gbuf_a", 4), ("gbuf_b", 4), ("hdr", 4), ("gbuf_c", 2), ("object_id", 2), ("keys", 2)):
        assert call(t=targets(**{name: off(a, by)})) == E and "misaligned" in urlib.ur_last_error().decode(), name
    assert call(rows=0) == E and call(row0=1, rows=64) == E and call(row0=64, rows=1) == E and call(row0=0xFFFFFFFF, rows=2) == E
    assert call(bits=32) == E and "key_triangle_bits" in urlib.ur_last_error().decode()
    assert call(d=draws(command_count=16), bits=28) == E and call(d=draws(command_count=2), bits=31) == E  # command_count >= 2^(32 - T)
    assert call(d=draws(command_count=1 << 24)) == lib.UR_EUNSUPPORTED and call(d=draws(command_count=0xFFFFFFFF)) == lib.UR_EUNSUPPORTED
    assert call(d=draws(command_count=1 << 24), bits=9) == E
    # ur_gbuffer_pass_parts: the same checks in either part, and the parts word itself
    g = urlib.ur_gbuffer_pass_parts
    parts = lambda parts_, t=tg, rows=64: g(ctx, v, p, C.byref(ok), depth, C.byref(t), 64, 64, 0, rows, 0, 0, st, parts_)  # noqa: E731
    assert (lib.UR_GBUFFER_PART_RASTER, lib.UR_GBUFFER_PART_RESOLVE) == (1, 2)
    assert re.search(r"#define UR_GBUFFER_PART_RASTER 0x1u", header) and re.search(r"#define UR_GBUFFER_PART_RESOLVE 0x2u", header)
    for bad in (0, 4, 7, 0x80000001):
        assert parts(bad) == E and "parts" in urlib.ur_last_error().decode(), bad
    for part in (1, 2, 3):
        assert parts(part, rows=0) == E and parts(part, t=targets(gbuf_a=None)) == E and parts(part, t=targets(keys=None)) == E, part
    del buf


def test_srgb_encode_table_is_the_documented_one():
    from unclerenderer_amd import hostmath
    t = hostmath.srgb_encode_table()
    assert t.shape == (255,) and t.dtype == np.float32 and (np.diff(t) > 0).all()
    assert t[0] == np.float32(0.5 / 255.0 / 12.92) and abs(float(t[254]) - ((254.5 / 255 + 0.055) / 1.055) ** 2.4) < 1e-7


def test_frame_gbuffer_pass_argument_checks(urlib):
    """ur_frame_set_gbuffer_pass and ur_frame_render's checks of the flag on a frame made over a stand-in context."""
    from unclerenderer_amd import lib
    buf, base, ctx = _stand_ins()
    E = lib.UR_EINVAL
    depth, cmds, idx, cnt, st, a, b, c, hdr, oid, keys, other = (C.c_void_p(base + 4096 * k) for k in range(1, 13))
    assert urlib.ur_frame_set_gbuffer_pass(None, None) == E
    f = C.c_void_p(urlib.ur_frame_create(ctx, None, 2, 0, 1))
    assert f.value

    def gp(stats=st, flags=0, bits=0, tg=None, **kw):
        d = lib.RasterDraws(cmds, 4, None, None, 0, None)
        for k, v in kw.items():
            setattr(d, k, v)
        return lib.FrameGBufferPass(d, tg if tg is not None else lib.GBufferTargets(a, b, c, hdr, oid, keys), stats, flags, bits)

    set_pass = urlib.ur_frame_set_gbuffer_pass
    for hole in range(4):
        t = [a, b, c, hdr]
        t[hole] = None
        assert set_pass(f, C.byref(gp(tg=lib.GBufferTargets(*t, oid, keys)))) == E
    assert set_pass(f, C.byref(gp(tg=lib.GBufferTargets(a, b, c, hdr, oid, None)))) == E
    assert set_pass(f, C.byref(gp(tg=lib.GBufferTargets(C.c_void_p(a.value + 4), b, c, hdr, oid, keys)))) == E
    assert set_pass(f, C.byref(gp(visible_idx=idx))) == E
    assert set_pass(f, C.byref(gp(commands=None))) == E
    assert set_pass(f, C.byref(gp(stats=C.c_void_p(st.value + 2)))) == E
    assert set_pass(f, C.byref(gp(flags=2))) == E and "flag" in urlib.ur_last_error().decode()
    assert set_pass(f, C.byref(gp(bits=32))) == E

    res = lib.FrameResources()
    res.width, res.height, res.row0, res.rows = 64, 32, 0, 32
    res.depth_full, res.gbuffer_a, res.gbuffer_b, res.gbuffer_c, res.lighting_band = depth, a, b, c, hdr
    consts = (C.c_uint32 * lib.UR_CULL_CONSTANT_DWORDS)()
    scene, sky = lib.SceneConstants(), lib.SkyConstants()
    G = lib.UR_FRAME_GBUFFER_PASS
    flags = lib.UR_FRAME_DEFAULT | lib.UR_FRAME_DEPTH_PASS | G
    render = lambda fl: urlib.ur_frame_render(f, C.byref(res), consts, C.byref(scene), C.byref(sky), fl)  # noqa: E731
    err = lambda: urlib.ur_last_error().decode()  # noqa: E731
    dpass = lambda fl=0: lib.FrameDepthPass(lib.RasterDraws(cmds, 4, None, None, 0, None), depth, st, fl)  # noqa: E731
    assert urlib.ur_frame_set_depth_pass(f, C.byref(dpass())) == lib.UR_OK
    assert render(lib.UR_FRAME_DEFAULT | G) == E and "UR_FRAME_DEPTH_PASS" in err()          # the flag without the depth pass' flag
    assert render(flags) == E and "ur_frame_set_gbuffer_pass" in err()                        # the flag without a pass
    assert set_pass(f, C.byref(gp(flags=lib.UR_DEPTH_QUANTIZE_D24))) == lib.UR_OK
    assert render(flags) == E and "quantise" in err()                                         # D24 in one pass only
    for hole in range(4):                                                                     # targets that are not the resources'
        t = [a, b, c, hdr]
        t[hole] = other
        assert set_pass(f, C.byref(gp(tg=lib.GBufferTargets(*t, oid, keys)))) == lib.UR_OK
        assert render(flags) == E and "same buffers" in err(), hole
    assert set_pass(f, None) == lib.UR_OK
    assert render(flags) == E and "ur_frame_set_gbuffer_pass" in err()
    urlib.ur_frame_destroy(f)
    del buf
