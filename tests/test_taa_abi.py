"""TemporalAA in the frame without a GPU: the new symbols, struct layouts, flags and argument checks (ur_temporal_aa_tonemap,
ur_frame_set_taa / reset_taa / taa_next, UR_FRAME_TAA / FUSE_TAA_TONEMAP), and the gfx950 code of the strip kernel's three forms."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import pytest

from tests.code_objects import LLVM, code_objects, kernel_metadata

ROOT = Path(__file__).resolve().parent.parent
NEW = ("ur_temporal_aa_tonemap", "ur_frame_set_taa", "ur_frame_reset_taa", "ur_frame_taa_next", "ur_host_taa_jitter", "ur_host_apply_taa_jitter")


def test_flags_do_not_collide():
    from unclerenderer_amd import lib
    new = {"UR_FRAME_TAA": 0x800000, "UR_FRAME_FUSE_TAA_TONEMAP": 0x1000000}
    for k, v in new.items():
        assert getattr(lib, k) == v
    old = [getattr(lib, n) for n in dir(lib) if n.startswith("UR_FRAME_") and n not in new and n != "UR_FRAME_DEFAULT"]
    assert len(old) >= 22
    for v in new.values():
        assert all(v & o == 0 for o in old)
    header = (ROOT / "include" / "ur_frame.h").read_text()
    defined = {m.group(1): int(m.group(2), 16) for m in re.finditer(r"#define (UR_FRAME_\w+) 0x([0-9a-fA-F]+)u", header)}
    assert {k: defined[k] for k in new} == new
    assert len(set(defined.values())) == len(defined)
    assert lib.UR_FRAME_DEFAULT & (lib.UR_FRAME_TAA | lib.UR_FRAME_FUSE_TAA_TONEMAP) == 0
    assert lib.UR_OPT_TAA_TONEMAP_HISTORY_STORE == int(re.search(r"#define UR_OPT_TAA_TONEMAP_HISTORY_STORE (\d+)", (ROOT / "include" / "ur_hotpath.h").read_text()).group(1))


def test_struct_layouts_match_the_header():
    from unclerenderer_amd import lib
    assert C.sizeof(lib.FrameTaa) == 16 and lib.FrameTaa.history_count.offset == 8 and lib.FrameTaa.history_weight.offset == 12
    assert C.sizeof(lib.FrameTaaInfo) == 20 and lib.FrameTaaInfo.jitter.offset == 12
    text = (ROOT / "include" / "ur_frame.h").read_text()

    def fields(name):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        return [re.findall(r"(\w+)\s*(?:\[\d+\])?\s*$", part.strip())[0] for decl in body.split(";") if decl.strip() for part in decl.split(",")]

    assert fields("ur_frame_taa") == [n for n, _ in lib.FrameTaa._fields_]
    assert fields("ur_frame_taa_info") == [n for n, _ in lib.FrameTaaInfo._fields_]


def test_symbols_declared_exported_and_bound(urlib):
    from unclerenderer_amd import hostmath, lib
    from unclerenderer_amd.hotpath import Frame, HotPath
    text = "".join(re.sub(r"/\*.*?\*/", "", (ROOT / "include" / h).read_text(), flags=re.S) for h in ("ur_hotpath.h", "ur_frame.h", "ur_host.h"))
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in lib.SIGNATURES and getattr(urlib, name) is not None
    for cls, names in ((HotPath, ("temporal_aa_tonemap",)), (Frame, ("set_taa", "taa_next", "reset_taa")), (hostmath, ("taa_jitter", "apply_taa_jitter"))):
        for n in names:
            assert callable(getattr(cls, n)), n
    if not (LLVM / "llvm-readelf").exists():
        pytest.skip("llvm tools not found")
    dyn = subprocess.run([str(LLVM / "llvm-readelf"), "--dyn-syms", "--wide", str(lib.library_path())], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert re.search(r"FUNC\s+GLOBAL\s+DEFAULT\s+\d+\s+%s$" % name, dyn, re.M), name


def test_fused_launch_argument_checks(urlib):
    from unclerenderer_amd import lib
    tm = lib.TonemapConstants(1, 0, 0.9, 2.2)
    buf = (C.c_uint64 * 8192)()
    base = C.addressof(buf)
    p, q, r, s = (C.c_void_p(base + k * 8192) for k in range(4))
    E = lib.UR_EINVAL
    f = urlib.ur_temporal_aa_tonemap
    assert f(None, C.byref(tm), p, q, r, None, s, 0.9, 1, 16, 16, 0, 16) == E  # null context
    assert "null" in urlib.ur_last_error().decode()
    # bad arguments are rejected before anything touches the context (a stand-in that is never dereferenced)
    ctx = C.c_void_p(base + 60000)
    assert f(ctx, None, p, q, r, None, s, 0.9, 1, 16, 16, 0, 16) == E          # no constants
    assert f(ctx, C.byref(tm), None, q, r, None, s, 0.9, 1, 16, 16, 0, 16) == E  # no current frame
    assert f(ctx, C.byref(tm), p, None, r, None, s, 0.9, 1, 16, 16, 0, 16) == E  # history wanted, none given
    assert f(ctx, C.byref(tm), p, q, None, None, s, 0.9, 1, 16, 16, 0, 16) == E  # no history output
    assert f(ctx, C.byref(tm), p, q, r, None, None, 0.9, 1, 16, 16, 0, 16) == E  # no LDR output
    assert f(ctx, C.byref(tm), p, q, r, None, s, 0.9, 1, 16, 16, 8, 9) == E      # out of the frame
    assert f(ctx, C.byref(tm), p, q, r, None, s, 0.9, 1, 0, 16, 0, 0) == E       # empty frame
    assert "ur_temporal_aa_tonemap" in urlib.ur_last_error().decode()
    assert f(ctx, C.byref(tm), p, None, r, None, s, 0.9, 0, 16, 16, 4, 0) == lib.UR_OK  # an empty band launches nothing
    # the store-hint option is a pair like the other launch-shape options
    assert urlib.ur_set_option(None, lib.UR_OPT_TAA_TONEMAP_HISTORY_STORE, 1) == E


def test_frame_ring_argument_checks(urlib):
    """ur_frame_set_taa / taa_next / render's TAA checks on frames made over a stand-in context: every check below returns before
    the context or a device pointer is used."""
    from unclerenderer_amd import lib
    buf = (C.c_uint64 * 8192)()
    base = C.addressof(buf)
    ctx = C.c_void_p(base + 60000)
    E, U = lib.UR_EINVAL, lib.UR_EUNSUPPORTED
    info = lib.FrameTaaInfo()
    assert urlib.ur_frame_set_taa(None, None) == E
    assert urlib.ur_frame_taa_next(None, C.byref(info)) == E
    urlib.ur_frame_reset_taa(None)  # a no-op, like ur_frame_reset_post(NULL)

    def ring(n, hole=None):
        ptrs = (C.c_void_p * max(n, 1))(*[None if k == hole else base + 4096 * (k + 1) for k in range(n)])
        t = lib.FrameTaa(C.cast(ptrs, C.POINTER(C.c_void_p)), n, 0.9)
        t._keep = ptrs
        return t

    for fif, n in ((3, 3), (1, 1), (2, 2), (0, 1)):  # 0 frames in flight count as 1 (max(1, FrameCount))
        f = C.c_void_p(urlib.ur_frame_create(ctx, None, fif, 0, 1))
        assert f
        try:
            assert urlib.ur_frame_taa_next(f, C.byref(info)) == E and "ring" in urlib.ur_last_error().decode()
            assert urlib.ur_frame_taa_next(f, None) == E
            for bad in (n + 1, n - 1, 0):
                assert urlib.ur_frame_set_taa(f, C.byref(ring(bad))) == E, (fif, bad)  # count != frames in flight
            assert "in flight" in urlib.ur_last_error().decode()
            assert urlib.ur_frame_set_taa(f, C.byref(ring(n, hole=n - 1))) == E           # a null slot
            assert "null" in urlib.ur_last_error().decode()
            assert urlib.ur_frame_set_taa(f, C.byref(lib.FrameTaa(None, n, 0.9))) == E    # no array
            res = lib.FrameResources()
            res.width, res.height, res.row0, res.rows = 16, 16, 0, 16
            res.tonemap_band = base
            cc = (C.c_uint32 * lib.UR_CULL_CONSTANT_DWORDS)()
            scene, sky = lib.SceneConstants(), lib.SkyConstants()
            TAA, FUSE, TM = lib.UR_FRAME_TAA, lib.UR_FRAME_FUSE_TAA_TONEMAP, lib.UR_FRAME_TONEMAP

            def render(flags):
                return urlib.ur_frame_render(f, C.byref(res), cc, C.byref(scene), C.byref(sky), flags)

            assert render(TM | TAA) == E and "ur_frame_set_taa" in urlib.ur_last_error().decode()  # no ring yet
            assert urlib.ur_frame_set_taa(f, C.byref(ring(n))) == lib.UR_OK
            # the first frame: slot 1 of N (the slot advances before the frame reads it), no history, no jitter
            assert urlib.ur_frame_taa_next(f, C.byref(info)) == lib.UR_OK
            assert (info.write_slot, info.read_slot, info.use_history) == (1 % n, (1 + n - 1) % n, 0)
            assert (info.jitter[0], info.jitter[1]) == (0.0, 0.0)
            assert render(TAA) == E                                            # TAA without TONEMAP
            assert render(TM | FUSE) == E                                      # the fuse flag without TAA
            assert render(TM | TAA | FUSE | lib.UR_FRAME_CAS | lib.UR_FRAME_FUSE_TONEMAP_CAS) == E  # both fuse flags
            assert "exclude" in urlib.ur_last_error().decode()
            res.rows = 8
            assert render(TM | TAA) == U                                       # a band
            res.row0, res.rows = 8, 8
            assert render(TM | TAA | FUSE) == U
            res.row0, res.rows = 0, 16
            assert render(TM | TAA | lib.UR_FRAME_POST_EXCHANGE) == U          # the post exchange
            assert "whole frame" in urlib.ur_last_error().decode()
            res.tonemap_band = None
            assert render(TM | TAA) == E                                       # no tonemap_band
            res.tonemap_band = base
            assert urlib.ur_frame_set_taa(f, None) == lib.UR_OK                # NULL clears
            assert urlib.ur_frame_taa_next(f, C.byref(info)) == E
            assert render(TM | TAA) == E
        finally:
            urlib.ur_frame_destroy(f)


def test_strip_kernels_use_no_scratch(urlib, tmp_path, record_property):
    """The gfx950 code of taa_strip_kernel: the plain form (ur_temporal_aa) and the two Tonemap forms (ur_temporal_aa_tonemap with
    either history-store hint) have no scratch and spill neither VGPRs nor SGPRs. The register counts are recorded, not asserted."""
    from unclerenderer_amd import lib
    if not (LLVM / "llvm-readelf").exists():
        pytest.skip("llvm tools not found")
    meta = {}
    for co in code_objects(lib.library_path(), tmp_path):
        meta.update({k: v for k, v in kernel_metadata(co).items() if "taa_strip_kernel" in k})
    assert len(meta) == 3, sorted(meta)
    assert sum("TonemapPost" in k for k in meta) == 2 and sum("NoPost" in k for k in meta) == 1, sorted(meta)
    for name, m in meta.items():
        record_property(name + ".vgpr_count", m["vgpr_count"])
        record_property(name + ".sgpr_count", m["sgpr_count"])
        print(name, m)
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
