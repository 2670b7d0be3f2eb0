"""The AutoExposure / CAS / fused Tonemap+CAS C-ABI without a GPU: struct layouts, exported symbols, argument checks, the frame
flags, the gfx950 code of the new kernels, and known answers of the scalar restatement the GPU tests compare against
(tests/post_ref.py)."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import post_ref
from tests.code_objects import LLVM, library_kernels

ROOT = Path(__file__).resolve().parent.parent
F = np.float32


def test_struct_layouts():
    from unclerenderer_amd import lib
    A = lib.AutoExposureConstants
    assert C.sizeof(A) == 36
    assert [(n, getattr(A, n).offset) for n, _ in A._fields_] == [
        ("InputSize", 0), ("DeltaTime", 8), ("AdaptationSpeedUp", 12), ("AdaptationSpeedDown", 16), ("UseHistory", 20),
        ("AutoExposureKey", 24), ("AutoExposureMin", 28), ("AutoExposureMax", 32)]
    K = lib.CasConstants
    assert C.sizeof(K) == 16
    assert [(n, getattr(K, n).offset) for n, _ in K._fields_] == [("TexelDelta", 0), ("Sharpness", 8), ("Padding", 12)]
    P = lib.FramePost
    assert C.sizeof(P) == 64 and P.tonemap_scratch.offset == 16 and P.delta_time.offset == 24 and P.cas_sharpness.offset == 56


def test_struct_layouts_match_the_header():
    """The C structs in include/ur_hotpath.h / ur_frame.h list the same fields in the same order as the ctypes ones."""
    from unclerenderer_amd import lib
    text = (ROOT / "include" / "ur_hotpath.h").read_text() + (ROOT / "include" / "ur_frame.h").read_text()

    def fields(name):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        out = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                for part in decl.split(",")[0:]:
                    out.append(re.findall(r"(\w+)\s*(?:\[\d+\])?\s*$", part.strip())[0])
        return out

    assert fields("ur_auto_exposure_constants") == [n for n, _ in lib.AutoExposureConstants._fields_]
    assert fields("ur_cas_constants") == [n for n, _ in lib.CasConstants._fields_]
    assert fields("ur_frame_post") == [n for n, _ in lib.FramePost._fields_]


def test_symbols_declared_and_exported(urlib):
    from unclerenderer_amd import lib
    for name in ("ur_auto_exposure", "ur_cas", "ur_tonemap_cas", "ur_frame_set_post", "ur_frame_reset_post"):
        assert name in lib.SIGNATURES
        assert getattr(urlib, name) is not None
    if not (LLVM / "llvm-readelf").exists():
        pytest.skip("llvm tools not found")
    dyn = subprocess.run([str(LLVM / "llvm-readelf"), "--dyn-syms", "--wide", str(lib.library_path())], capture_output=True, text=True, check=True).stdout
    for name in ("ur_auto_exposure", "ur_cas", "ur_tonemap_cas", "ur_frame_set_post", "ur_frame_reset_post"):
        assert re.search(r"FUNC\s+GLOBAL\s+DEFAULT\s+\d+\s+%s$" % name, dyn, re.M), name


def test_null_context_and_bad_arguments_are_rejected(urlib):
    from unclerenderer_amd import lib
    ae = lib.AutoExposureConstants((C.c_float * 2)(16, 16), 0.0, 3.0, 1.0, 0, 0.3, 0.1, 5.0)
    cas = lib.CasConstants((C.c_float * 2)(1 / 16, 1 / 16), 0.5, 0.0)
    tm = lib.TonemapConstants(1, 0, 0.9, 2.2)
    buf = (C.c_uint32 * 256)()
    p = C.cast(buf, C.c_void_p)
    assert urlib.ur_auto_exposure(None, C.byref(ae), p, 16, 16, None, p) == lib.UR_EINVAL
    assert urlib.ur_cas(None, C.byref(cas), p, p, 16, 16, 0, 16) == lib.UR_EINVAL
    assert urlib.ur_tonemap_cas(None, C.byref(tm), C.byref(cas), p, None, p, 16, 16, 0, 16) == lib.UR_EINVAL
    assert urlib.ur_frame_set_post(None, None) == lib.UR_EINVAL
    assert "null" in urlib.ur_last_error().decode()
    urlib.ur_frame_reset_post(None)  # a no-op, like ur_frame_reset_hzb(NULL)


def test_frame_flags_do_not_collide():
    from unclerenderer_amd import lib
    new = {"UR_FRAME_AUTO_EXPOSURE": 0x40000, "UR_FRAME_CAS": 0x80000, "UR_FRAME_FUSE_TONEMAP_CAS": 0x100000}
    for k, v in new.items():
        assert getattr(lib, k) == v
    old = [getattr(lib, n) for n in dir(lib) if n.startswith("UR_FRAME_") and n not in new and n != "UR_FRAME_DEFAULT"]
    assert len(old) >= 17
    for v in new.values():
        assert all(v & o == 0 for o in old)
    header = (ROOT / "include" / "ur_frame.h").read_text()
    defined = {m.group(1): int(m.group(2), 16) for m in re.finditer(r"#define (UR_FRAME_\w+) 0x([0-9a-fA-F]+)u", header)}
    assert {k: defined[k] for k in new} == new
    assert len(set(defined.values())) == len(defined)


def test_post_kernels_use_no_scratch(urlib, tmp_path):
    """The gfx950 code of the AutoExposure and CAS kernels (all four strip forms) has no scratch and no spills."""
    if not (LLVM / "llvm-readelf").exists():
        pytest.skip("llvm tools not found")
    meta = library_kernels(tmp_path)
    post = {k: v for k, v in meta.items() if "cas_strip_kernel" in k or "auto_exposure_kernel" in k}
    assert len(post) == 5, sorted(post)
    for name, m in post.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)


# ---- known answers of the restatement -------------------------------------------------------------------------------------

def _flat(h, w, rgb):
    img = np.zeros((h, w, 4), F)
    img[..., :3] = rgb
    img[..., 3] = 1
    return img


def test_ae_constant_luminance_is_exact():
    for (h, w), v in (((9, 17), 0.25), ((131, 257), 3.0), ((1080, 1920), 0.0371)):
        img = _flat(h, w, v)
        L = F(F(F(v) * post_ref.LUM[0] + F(v) * post_ref.LUM[1]) + F(v) * post_ref.LUM[2])
        want = np.minimum(np.maximum(F(np.log2(F(0.3)) - np.log2(L)), np.log2(F(0.1))), np.log2(F(5.0)))
        assert post_ref.auto_exposure(img) == want
    # both clamp bounds
    assert post_ref.auto_exposure(_flat(8, 8, 100.0)) == np.log2(F(0.1))
    assert post_ref.auto_exposure(_flat(8, 8, 0.001)) == np.log2(F(5.0))


def test_ae_one_history_step():
    target = post_ref.auto_exposure(_flat(16, 16, 0.5))
    prev = F(target - 1.0)  # target > prev: speed up
    got = post_ref.auto_exposure(_flat(16, 16, 0.5), prev=prev, use_history=True, delta_time=1 / 60, speed_up=3.0, speed_down=1.0)
    a = 1.0 - np.exp(-0.05)
    assert abs(float(got) - (float(prev) + a * (float(target) - float(prev)))) < 1e-6


def test_ae_speed_down_when_target_not_above_prev():
    target = post_ref.auto_exposure(_flat(16, 16, 0.5))
    for prev in (F(target + 0.75), F(target)):
        got = post_ref.auto_exposure(_flat(16, 16, 0.5), prev=prev, use_history=True, delta_time=0.1, speed_up=7.0, speed_down=0.5)
        a = 1.0 - np.exp(-0.1 * 0.5)
        assert abs(float(got) - (float(prev) + a * (float(target) - float(prev)))) < 1e-6


def test_ae_nan_texel_counts_as_zero():
    img = _flat(32, 32, 0.5)
    # the tap of lane (0, 0) samples around (1, 1) - 0.5 = (0.5, 0.5): the footprint is texels (0..1, 0..1)
    img[0, 0, 0] = np.nan
    assert np.isfinite(post_ref.auto_exposure(img))
    assert post_ref.auto_exposure(img) > post_ref.auto_exposure(_flat(32, 32, 0.5))  # a darker tap: a higher exposure


def _pack(r, g, b):
    return (np.asarray(r, np.uint32) | (np.asarray(g, np.uint32) << 8) | (np.asarray(b, np.uint32) << 16) | np.uint32(0xFF000000)).astype(np.uint32)


def test_cas_flat_image_is_unchanged():
    rng = np.random.default_rng(3)
    for _ in range(8):
        r, g, b = rng.integers(0, 256, 3)
        img = np.full((7, 9), _pack(r, g, b), np.uint32)
        for s in (0.0, 0.5, 1.0):
            assert np.array_equal(post_ref.cas(img, s), img)


def test_cas_sharpness_zero_returns_the_input():
    rng = np.random.default_rng(4)
    img = _pack(*rng.integers(0, 256, (3, 33, 47)))
    assert np.array_equal(post_ref.cas(img, 0.0), img)


def test_cas_step_edge_is_clamped():
    img = np.where(np.arange(16)[None, :] < 8, _pack(0, 0, 0), _pack(255, 255, 255)) * np.ones((6, 1), np.uint32)
    assert np.array_equal(post_ref.cas(img.astype(np.uint32), 1.0), img)  # 0 cannot go below 0 nor 255 above 255
    grey = np.where(np.arange(16)[None, :] < 8, _pack(64, 64, 64), _pack(192, 192, 192)) * np.ones((6, 1), np.uint32)
    out = post_ref.bytes_of(post_ref.cas(grey.astype(np.uint32), 1.0))
    assert (out[:, 7, :3] < 64).all() and (out[:, 8, :3] > 192).all()  # the edge is steepened ...
    assert (out[:, :6, :3] == 64).all() and (out[:, 10:, :3] == 192).all()  # ... and flat areas are left alone
    assert (out[..., 3] == 255).all()


def test_cas_band_rows_equal_full_rows():
    rng = np.random.default_rng(5)
    img = _pack(*rng.integers(0, 256, (3, 21, 13)))
    full = post_ref.cas(img, 0.5)
    for r0, n in ((0, 1), (0, 5), (9, 3), (20, 1)):
        assert np.array_equal(post_ref.cas(img, 0.5, r0, n), full[r0:r0 + n])
