"""The ABI of the sky capture without a GPU (include/ur_env_sky.h): the header against a compiled probe, the symbols
declared, exported and bound, every refusal of ur_env_sky, ur_host_env_sky and ur_host_env_sky_params - decided before a device is
needed - the Python functions' refusals, the host units of the capture and of the BRDF LUT built by the plain host compiler, the host
builds and the kernels' waves under ASan / UBSan in a stand-alone program (tests/cpp/env_sky_main.cpp), and the two new kernels'
resources from the built library's metadata, read by tests/code_objects_named.py (the kernels have C linkage: plain names)."""
import ctypes as C
import json
import math
import re
import subprocess

import numpy as np
import pytest

from tests import env_sky_ref as R
from tests.test_bcn_abi import ROOT, _cxx

CSRC = ROOT / "unclerenderer_amd" / "csrc"
HOST_UNITS = [str(CSRC / n) for n in ("env_sky_host.cpp", "brdf_lut_host.cpp")]
NEW = {"ur_env_sky": "ur_env_sky.h", "ur_host_env_sky": "ur_host.h", "ur_host_env_sky_params": "ur_host.h", "ur_brdf_lut": "ur_brdf_lut.h",
       "ur_brdf_lut_table_bytes": "ur_brdf_lut.h", "ur_host_brdf_lut": "ur_host.h", "ur_host_brdf_lut_table": "ur_host.h"}
NEW_KERNELS = ("ur_env_sky_kernel", "ur_brdf_lut_kernel")


def test_header_against_a_compiled_probe(tmp_path):
    from unclerenderer_amd import lib
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ur_env_sky.h"\n#include "ur_host.h"\n'
                   'int main(void) { printf("%u %u %u %zu %zu %zu %zu\\n", UR_ENV_SKY_MAX_BASE_SIZE, UR_ENV_SKY_MAX_TAPS, UR_ENV_SKY_MAX_STREAM_OPS, sizeof(ur_sky_constants), '
                   "offsetof(ur_sky_constants, CameraPosition), offsetof(ur_sky_constants, LightDirection), offsetof(ur_sky_constants, LightColor)); "
                   "int (*run)(ur_ctx*, const ur_sky_constants*, uint32_t, uint32_t, void*, size_t) = ur_env_sky; "
                   "int (*twin)(const ur_sky_constants*, uint32_t, uint32_t, void*, size_t) = ur_host_env_sky; "
                   "int (*fold)(const ur_sky_constants*, float*) = ur_host_env_sky_params; (void)run; (void)twin; (void)fold; return 0; }\n")
    stub = tmp_path / "stub.c"  # (the probe takes the entry point's address: the host units have the rest, a stub stands for the device call)
    stub.write_text('#include "ur_env_sky.h"\nint ur_env_sky(ur_ctx* c, const ur_sky_constants* k, uint32_t b, uint32_t t, void* d, size_t n)\n'
                    "{ (void)c; (void)k; (void)b; (void)t; (void)d; (void)n; return 0; }\n")
    so, exe = tmp_path / "libhost.so", tmp_path / "probe"
    cc = _cxx().replace("g++", "gcc").replace("c++", "cc")
    subprocess.run([_cxx(), "-std=c++17", "-shared", "-fPIC"] + HOST_UNITS + ["-o", str(so)], check=True)
    subprocess.run([cc, "-std=c99", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}", str(src), str(stub), str(so), f"-Wl,-rpath,{tmp_path}", "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [2048, 16, 1, 240, 192, 208, 224]
    assert got[:3] == [lib.UR_ENV_SKY_MAX_BASE_SIZE, lib.UR_ENV_SKY_MAX_TAPS, lib.UR_ENV_SKY_MAX_STREAM_OPS]
    assert [getattr(lib.SkyConstants, n).offset for n in ("CameraPosition", "LightDirection", "LightColor")] == got[4:]


def test_symbols_declared_exported_and_bound(urlib):
    from unclerenderer_amd import build, environment, hostmath, hotpath, lib
    strip = lambda text: re.sub(r"/\*.*?\*/", "", text, flags=re.S)  # noqa: E731
    for name, header in NEW.items():
        assert re.search(r"\b%s\s*\(" % name, strip((ROOT / "include" / header).read_text())), name
        assert name in lib.SIGNATURES and getattr(urlib, name) is not None
    for fn in (environment.sky_to_cube, environment.bake_sky, environment.brdf_lut, hostmath.env_sky, hostmath.env_sky_params, hostmath.brdf_lut, hostmath.brdf_lut_table):
        assert callable(fn)
    # nothing new on HotPath, Frame or the hotpath package; nothing wired into the frame or the hot path's header
    for owner in (hotpath.HotPath, hotpath.Frame, hotpath):
        assert not [n for n in dir(owner) if "env_sky" in n.lower() or "bake_sky" in n.lower() or "brdf_lut" in n.lower()], owner
    for header in ("ur_frame.h", "ur_hotpath.h"):
        text = strip((ROOT / "include" / header).read_text())
        assert "ur_env_sky" not in text and "ur_brdf_lut" not in text
    flags = dict(build.SOURCES)
    assert flags["env_sky.hip"] == build.EXACT and flags["brdf_lut.hip"] == build.EXACT
    assert "-ffp-contract=off" in flags["env_sky_host.cpp"] and "-ffp-contract=off" in flags["brdf_lut_host.cpp"]
    # the device units name no libm function but sqrtf, which is an instruction; the rules' own saturate and fold (host only: exp, sqrt
    # in double) aside, and no approximation of lighting_device.h
    for unit, rule in (("env_sky.hip", "env_sky_rule.h"), ("brdf_lut.hip", "brdf_lut_rule.h")):
        device = re.sub(r"//.*", "", (CSRC / unit).read_text() + (CSRC / rule).read_text())
        device = re.sub(r"inline Params fold\(.*?\n}\n", "", device, flags=re.S)
        assert not re.search(r"\b(atan2?f?|sinf?|cosf?|tanf?|asinf?|acosf?|log2?f?|powf?|expf?|ldexpf?|frexpf?|__sinf|__cosf|rcp|rsq|__frcp_rn|__fsqrt_rn)\s*\(", device), unit
        assert 'extern "C" __global__' in (CSRC / unit).read_text() and "template" not in device


def test_the_host_units_build_with_the_plain_compiler_and_build_the_same(tmp_path, urlib):
    so = tmp_path / "libenv_sky_host.so"
    subprocess.run([_cxx(), "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC"] + HOST_UNITS + ["-o", str(so)], check=True)
    from unclerenderer_amd import hostmath
    plain = C.CDLL(str(so))
    for sun, base, taps in (((0.3, 0.8, -0.5), 8, 4), ((0, -1, 0), 16, 1), ((-40, 2, 9), 4, 16)):
        sky = R.sky_constants(sun, camera_y=700.0)
        assert np.array_equal(hostmath.env_sky(sky, base, taps), hostmath.env_sky(sky, base, taps, library=plain))
    for w, h, s in ((7, 5, 64), (64, 8, 16), (16, 4, 1024)):
        table = hostmath.brdf_lut_table(h, s)
        assert np.array_equal(table, hostmath.brdf_lut_table(h, s, library=plain))
        assert np.array_equal(hostmath.brdf_lut(w, h, s, table=table), hostmath.brdf_lut(w, h, s, table=table, library=plain))


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    """tests/cpp/env_sky_main.cpp with the host units, built once with -fsanitize=address,undefined: its own main, no Python, no device."""
    exe = tmp_path_factory.mktemp("env_sky_sanitize") / "env_sky_main"
    subprocess.run([_cxx(), "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    str(ROOT / "tests" / "cpp" / "env_sky_main.cpp")] + HOST_UNITS + ["-o", str(exe)], check=True)
    return exe


@pytest.mark.parametrize("base,taps", [(1, 1), (1, 16), (2, 2), (4, 4), (4, 8), (2, 16), (8, 1), (16, 2)])
def test_sky_host_build_and_the_waves_under_asan_and_ubsan(sanitized, base, taps):
    """The host build into a heap buffer of exactly the cube's size, then the device's waves on the host (the functions the kernel calls),
    descending, whole workgroups, into a buffer that arrives as 0xFF: the same bytes, no access outside."""
    from unclerenderer_amd import hostmath
    sun, color, cam = (0.3, 0.8, -0.5), (1.0, 0.95, 0.9), 120.0
    r = subprocess.run([str(sanitized), "sky", str(base), str(taps), repr(cam)] + [repr(v) for v in sun + color], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
    want = hostmath.env_sky(R.sky_constants(sun, color, cam), base, taps)
    assert r.stdout.split() == ["0", str(int(want.view(np.uint8).sum(dtype=np.uint64)))]


@pytest.mark.parametrize("w,h,s", [(1, 1, 16), (3, 2, 64), (7, 5, 16), (64, 8, 64), (16, 4, 1024), (1024, 1, 16), (1, 256, 32)])
def test_lut_host_build_and_the_waves_under_asan_and_ubsan(sanitized, w, h, s):
    from unclerenderer_amd import hostmath
    r = subprocess.run([str(sanitized), "lut", str(w), str(h), str(s)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
    want = hostmath.brdf_lut(w, h, s)
    assert r.stdout.split() == ["0", str(int(want.view(np.uint8).sum(dtype=np.uint64)))]


def test_refusals_that_need_no_device(urlib):
    """Every check comes before the context is looked at: a stand-in context is enough, the address is a number and is not dereferenced.
    The host twin has the same refusals but for the context; the fold refuses the constants the capture refuses."""
    from unclerenderer_amd import lib
    stand_in = C.create_string_buffer(4096)
    base, taps = 16, 4
    ok = dict(ctx=C.addressof(stand_in), sky=R.sky_constants((0.3, 0.8, -0.5)), base=base, taps=taps, dst=0x300000, dst_bytes=48 * base * base)

    def refused(text, **kw):
        a = dict(ok, **kw)
        sky = C.byref(a["sky"]) if a["sky"] is not None else None
        rc, said = urlib.ur_env_sky(a["ctx"], sky, a["base"], a["taps"], a["dst"], a["dst_bytes"]), urlib.ur_last_error().decode()
        assert rc == lib.UR_EINVAL and text in said, (text, kw, rc, said)
        if "ctx" not in kw:
            assert urlib.ur_host_env_sky(sky, a["base"], a["taps"], a["dst"], a["dst_bytes"]) == lib.UR_EINVAL, kw

    refused("null context", ctx=None)
    refused("null constants", sky=None)
    refused("null destination", dst=None)
    for b in (0, 3, 12, 24, 4096, 1 << 31):
        refused(f"base size {b}", base=b)
    for k in (0, 3, 6, 12, 32, 64, 1 << 31):
        refused(f"{k} taps a side", taps=k)
    refused("destination bytes", dst_bytes=ok["dst_bytes"] - 8)
    refused("destination bytes", dst_bytes=ok["dst_bytes"] + 8)
    refused("destination bytes", base=32)  # another cube's size
    for off in (4, 8, 12):
        refused("destination not 16-byte aligned", dst=ok["dst"] + off)
    out = np.zeros(10, np.float32)
    for field, text in (("CameraPosition", "CameraPosition.y that is not finite"), ("LightDirection", "not finite"), ("LightColor", "not finite")):
        for bad in (math.inf, -math.inf, math.nan):
            for i in ((1,) if field == "CameraPosition" else (0, 1, 2)):
                sky = R.sky_constants((0.3, 0.8, -0.5))
                getattr(sky, field)[i] = bad
                refused(text, sky=sky)
                assert urlib.ur_host_env_sky_params(C.byref(sky), lib.fptr(out)) == lib.UR_EINVAL
    for zero in ((0.0, 0.0, 0.0), (-0.0, 0.0, -0.0)):
        refused("LightDirection of length zero", sky=R.sky_constants(zero))
        assert urlib.ur_host_env_sky_params(C.byref(R.sky_constants(zero)), lib.fptr(out)) == lib.UR_EINVAL
    assert urlib.ur_host_env_sky_params(None, lib.fptr(out)) == lib.UR_EINVAL and urlib.ur_host_env_sky_params(C.byref(ok["sky"]), None) == lib.UR_EINVAL
    # what is not read may hold anything: a camera's x and z and the matrices
    sky = R.sky_constants((1e-30, 0.0, 0.0))
    sky.CameraPosition[0], sky.CameraPosition[2], sky.View[3] = math.nan, math.inf, math.nan
    assert urlib.ur_host_env_sky_params(C.byref(sky), lib.fptr(out)) == 0 and list(out[:3]) == [1, 0, 0]


def test_python_functions_refuse(urlib):
    from unclerenderer_amd import environment, hostmath, hotpath

    class T:  # a stand-in for a device tensor: an address and a size
        is_cuda = True

        def __init__(self, address, nbytes):
            self.address, self.nbytes = address, nbytes

        def is_contiguous(self):
            return True

        def data_ptr(self):
            return self.address

        def numel(self):
            return self.nbytes

        def element_size(self):
            return 1

    class NoDevice(hotpath.HotPath):
        def __init__(self):
            self._L, self._ctx, self.device = urlib, None, 0
    hp = NoDevice()
    sky = R.sky_constants((0.3, 0.8, -0.5))
    for base, taps in ((0, 1), (24, 1), (4096, 1), (8, 3), (8, 32), (8, 0)):
        with pytest.raises(ValueError, match="no sky capture"):
            environment.sky_to_cube(hp, sky, base, taps, out=T(0x1000, 48 * base * base))
        with pytest.raises(ValueError, match="no sky capture"):
            environment.bake_sky(hp, sky, base, 64, taps)
        with pytest.raises(ValueError, match="ur_host_env_sky failed"):
            hostmath.env_sky(sky, base, taps)
    with pytest.raises(TypeError, match="lib.SkyConstants"):
        environment.sky_to_cube(hp, None, 8)
    with pytest.raises(ValueError, match="is 3072 bytes, out has 3064"):
        environment.sky_to_cube(hp, sky, 8, out=T(0x4000, 3064))
    for bad in (R.sky_constants((0, 0, 0)), R.sky_constants((math.nan, 1, 0)), R.sky_constants((0, 1, 0), (math.inf, 1, 1)), R.sky_constants((0, 1, 0), camera_y=math.nan)):
        with pytest.raises(ValueError, match="ur_host_env_sky_params failed"):
            environment.sky_to_cube(hp, bad, 8, out=T(0x4000, 3072))
        with pytest.raises(ValueError, match="ur_host_env_sky_params failed"):
            hostmath.env_sky_params(bad)
        with pytest.raises(ValueError, match="ur_host_env_sky failed"):
            hostmath.env_sky(bad, 8)
    cube = hostmath.env_sky(sky, 8, 2)
    assert cube.shape == (6, 8, 8, 4) and cube.dtype == np.uint16 and (cube[..., 3] == 0x3C00).all()


def test_new_kernels_use_no_scratch_and_the_old_ones_are_as_they_were(urlib, tmp_path):
    """The code objects' metadata notes. The two new kernels have C linkage and stand under their plain names; they have no scratch, spill
    nothing and stay within 64 VGPRs (DESIGN.md 3.22 records the counts). Every mangled kernel of the commit before
    (tests/golden/kernel_metadata_before_env_sky.json: private segment, SGPRs, spilled SGPRs, VGPRs, spilled VGPRs, recorded from that
    commit's library) is still there with the same figures, and there is no other."""
    from tests.code_objects_named import library_kernels
    kernels = library_kernels(tmp_path)
    new = {k: v for k, v in kernels.items() if not k.startswith("_Z")}
    assert sorted(new) == sorted(NEW_KERNELS), sorted(new)
    for name, meta in new.items():
        print(name, meta)
        assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0 and meta["sgpr_spill_count"] == 0, (name, meta)
        assert meta["vgpr_count"] <= 64, (name, meta)  # eight waves a SIMD
    before = json.loads((ROOT / "tests" / "golden" / "kernel_metadata_before_env_sky.json").read_text())
    keys = ("private_segment_fixed_size", "sgpr_count", "sgpr_spill_count", "vgpr_count", "vgpr_spill_count")
    assert len(before) == 143 and set(kernels) == set(before) | set(new)
    moved = {k: (v, [kernels.get(k, {}).get(f) for f in keys]) for k, v in before.items() if [kernels.get(k, {}).get(f) for f in keys] != v}
    assert not moved, moved
