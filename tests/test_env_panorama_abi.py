"""The ABI of the environment from a panorama without a GPU (include/ur_env_panorama.h, include/ur_assets.h): the headers
against a compiled probe, the symbols declared, exported and bound, every refusal of ur_env_panorama and ur_host_env_panorama - decided
before a device is needed - the Python functions' refusals, the host units built by the plain host compiler, the parser, the unpacker,
the host build and the kernel's waves under ASan / UBSan in a stand-alone program (tests/cpp/env_panorama_main.cpp), and the kernels'
resources from the built library's metadata."""
import ctypes as C
import json
import re
import subprocess

import numpy as np
import pytest

from tests import env_panorama_ref as R
from tests.test_bcn_abi import ROOT, _cxx

CSRC = ROOT / "unclerenderer_amd" / "csrc"
HOST_UNITS = [str(CSRC / n) for n in ("hdr.cpp", "env_panorama_host.cpp")]
NEW = {"ur_env_panorama": "ur_env_panorama.h", "ur_host_env_panorama": "ur_host.h", "ur_host_env_panorama_taps": "ur_host.h", "ur_hdr_parse": "ur_assets.h",
       "ur_hdr_unpack": "ur_assets.h", "ur_hdr_last_error": "ur_assets.h"}


def test_header_against_a_compiled_probe(tmp_path):
    from unclerenderer_amd import lib
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ur_env_panorama.h"\n#include "ur_assets.h"\n#include "ur_host.h"\n'
                   'int main(void) { printf("%u %u %u %u %u %u %u %zu %zu %zu %zu %zu %u %u\\n", UR_ENV_PANORAMA_MAX_WIDTH, UR_ENV_PANORAMA_MAX_HEIGHT, '
                   "UR_ENV_PANORAMA_MAX_BASE_SIZE, UR_ENV_PANORAMA_MAX_TAPS, UR_ENV_PANORAMA_MAX_STREAM_OPS, UR_HDR_MAX_WIDTH, UR_HDR_MAX_HEIGHT, sizeof(ur_hdr_info), "
                   "offsetof(ur_hdr_info, width), offsetof(ur_hdr_info, height), offsetof(ur_hdr_info, payload_offset), offsetof(ur_hdr_info, rle), "
                   "ur_host_env_panorama_taps(4096u, 2048u, 512u), ur_host_env_panorama_taps(4096u, 2048u, 3u)); "
                   "int (*run)(ur_ctx*, const void*, size_t, uint32_t, uint32_t, uint32_t, uint32_t, void*, size_t) = ur_env_panorama; "
                   "int (*twin)(const void*, size_t, uint32_t, uint32_t, uint32_t, uint32_t, void*, size_t) = ur_host_env_panorama; "
                   "int (*parse)(const void*, size_t, ur_hdr_info*) = ur_hdr_parse; int (*unpack)(const void*, size_t, const ur_hdr_info*, uint8_t*) = ur_hdr_unpack; "
                   "const char* (*said)(void) = ur_hdr_last_error; (void)run; (void)twin; (void)parse; (void)unpack; (void)said; return 0; }\n")
    stub = tmp_path / "stub.c"  # (the probe takes the entry point's address: the host units have the rest, a stub stands for the device call)
    stub.write_text('#include "ur_env_panorama.h"\nint ur_env_panorama(ur_ctx* c, const void* s, size_t n, uint32_t w, uint32_t h, uint32_t b, uint32_t k, void* d, size_t dn)\n'
                    "{ (void)c; (void)s; (void)n; (void)w; (void)h; (void)b; (void)k; (void)d; (void)dn; return 0; }\n")
    so, exe = tmp_path / "libhost.so", tmp_path / "probe"
    cc = _cxx().replace("g++", "gcc").replace("c++", "cc")
    subprocess.run([_cxx(), "-std=c++17", "-shared", "-fPIC"] + HOST_UNITS + ["-o", str(so)], check=True)
    subprocess.run([cc, "-std=c99", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}", str(src), str(stub), str(so), f"-Wl,-rpath,{tmp_path}", "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [16384, 8192, 2048, 16, 1, 16384, 8192, 16, 0, 4, 8, 12, 8, 0]
    assert got[:5] == [lib.UR_ENV_PANORAMA_MAX_WIDTH, lib.UR_ENV_PANORAMA_MAX_HEIGHT, lib.UR_ENV_PANORAMA_MAX_BASE_SIZE, lib.UR_ENV_PANORAMA_MAX_TAPS,
                       lib.UR_ENV_PANORAMA_MAX_STREAM_OPS]
    assert C.sizeof(lib.HdrInfo) == 16 and [getattr(lib.HdrInfo, n).offset for n in ("width", "height", "payload_offset", "rle")] == [0, 4, 8, 12]


def test_symbols_declared_exported_and_bound(urlib):
    from unclerenderer_amd import assets, build, environment, hostmath, hotpath, lib
    strip = lambda text: re.sub(r"/\*.*?\*/", "", text, flags=re.S)  # noqa: E731
    for name, header in NEW.items():
        assert re.search(r"\b%s\s*\(" % name, strip((ROOT / "include" / header).read_text())), name
        assert name in lib.SIGNATURES and getattr(urlib, name) is not None
    assert callable(environment.panorama_to_cube) and callable(environment.bake_panorama)
    assert callable(hostmath.env_panorama) and callable(hostmath.env_panorama_taps) and callable(assets.load_panorama_hdr) and callable(assets.parse_panorama_hdr)
    # nothing new on HotPath, Frame or the hotpath package; nothing wired into the frame or the hot path's header
    for owner in (hotpath.HotPath, hotpath.Frame, hotpath):
        assert not [n for n in dir(owner) if "panorama" in n.lower()], owner
    for header in ("ur_frame.h", "ur_hotpath.h"):
        assert "panorama" not in strip((ROOT / "include" / header).read_text())
    flags = dict(build.SOURCES)
    assert flags["env_panorama.hip"] == build.EXACT and "-ffp-contract=off" in flags["env_panorama_host.cpp"] and "hdr.cpp" in flags
    # the device unit names no libm function but sqrtf, fabsf, floorf and copysignf, which are instructions
    device = re.sub(r"//.*", "", (CSRC / "env_panorama.hip").read_text() + (CSRC / "env_panorama_rule.h").read_text())
    assert not re.search(r"\b(atan2?f?|sinf?|cosf?|tanf?|asinf?|acosf?|log2?f?|powf?|expf?|ldexpf?|frexpf?|__sinf|__cosf)\s*\(", device)


def test_the_host_units_build_with_the_plain_compiler_and_build_the_same(tmp_path, urlib):
    so = tmp_path / "libenv_panorama_host.so"
    subprocess.run([_cxx(), "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC"] + HOST_UNITS + ["-o", str(so)], check=True)
    from unclerenderer_amd import hostmath
    plain = C.CDLL(str(so))
    for w, h, base, taps in ((67, 33, 8, 4), (8, 4, 16, 1), (64, 32, 4, 16)):
        pano = R.random_panorama(w + base + taps, w, h)
        assert np.array_equal(hostmath.env_panorama(pano, w, h, base, taps), hostmath.env_panorama(pano, w, h, base, taps, library=plain))
    data = R.hdr_file(R.random_panorama(3, 40, 6), True)
    info, out = (C.c_uint32 * 4)(), np.zeros((6, 40, 4), np.uint8)
    assert plain.ur_hdr_parse(data, C.c_size_t(len(data)), info) == 0 and list(info)[:2] == [40, 6] and info[3] == 1
    assert plain.ur_hdr_unpack(data, C.c_size_t(len(data)), info, C.c_void_p(out.ctypes.data)) == 0 and np.array_equal(out, R.random_panorama(3, 40, 6))


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    """tests/cpp/env_panorama_main.cpp with the host units, built once with -fsanitize=address,undefined: its own main, no Python, no device."""
    exe = tmp_path_factory.mktemp("env_panorama_sanitize") / "env_panorama_main"
    subprocess.run([_cxx(), "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    str(ROOT / "tests" / "cpp" / "env_panorama_main.cpp")] + HOST_UNITS + ["-o", str(exe)], check=True)
    return exe


def test_texel_values_are_exact(sanitized):
    """Every (m, e) is m * 2^(e - 136) exactly; by hand: 1 * 2^-135 is 2^14 units of 2^-149, 3 * 2^-134 is 3 * 2^15 of them, 255 * 2^-127 is
    1.9921875 * 2^-120 (biased exponent 7), 128 * 2^-7 is 1.0, 255 * 2^119 is 1.9921875 * 2^126 (biased exponent 253)."""
    r = subprocess.run([str(sanitized), "values"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "values ok", (r.stdout[-1000:], r.stderr[-2000:])
    for (m, e), bits in (((1, 1), 0x00004000), ((3, 2), 0x00018000), ((255, 9), 0x03FF0000), ((128, 129), 0x3F800000), ((255, 255), 0x7EFF0000), ((7, 0), 0), ((0, 200), 0)):
        r = subprocess.run([str(sanitized), "value", str(m), str(e)], capture_output=True, text=True)
        assert r.returncode == 0 and int(r.stdout, 16) == bits, (m, e, r.stdout, r.stderr[-2000:])


@pytest.mark.parametrize("w,h,rle", [(67, 33, True), (67, 33, False), (8, 2, True), (3, 5, False), (200, 3, True)])
def test_parser_and_unpacker_under_asan_and_ubsan(sanitized, tmp_path, w, h, rle):
    """The test file and every prefix of it, each in a heap block of exactly its size, into a destination of exactly the image's size."""
    pano = R.random_panorama(w * h, w, h)
    path = tmp_path / "p.hdr"
    data = R.hdr_file(pano, rle)
    path.write_bytes(data)
    r = subprocess.run([str(sanitized), "file", str(path)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
    got = [int(v) for v in r.stdout.split()]
    assert got[:5] == [0, w, h, int(rle), int(pano.sum(dtype=np.uint64))]
    assert got[5] == len(data)  # the image ends with the file: every shorter file is refused


@pytest.mark.parametrize("w,h,base,taps", [(1, 1, 1, 1), (67, 33, 1, 1), (67, 33, 2, 2), (8, 4, 4, 4), (67, 33, 4, 8), (64, 32, 2, 16), (67, 33, 8, 1), (16384, 1, 4, 2),
                                           (1, 8192, 2, 4)])
def test_host_build_and_the_waves_under_asan_and_ubsan(sanitized, tmp_path, w, h, base, taps):
    """The host build from a heap buffer of exactly the panorama's size into one of exactly the cube's, then the device's waves on the host
    (the functions the kernel calls), descending, whole workgroups, into a buffer that arrives as 0xFF: the same bytes, no access outside."""
    from unclerenderer_amd import hostmath
    pano = R.random_panorama(11 * base + taps + w, w, h)
    blob = tmp_path / "pano.bin"
    blob.write_bytes(np.uint32([w, h, base, taps]).tobytes() + pano.tobytes())
    r = subprocess.run([str(sanitized), "build", str(blob)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
    want = hostmath.env_panorama(pano, w, h, base, taps)
    assert r.stdout.split() == ["0", str(int(want.view(np.uint8).sum(dtype=np.uint64)))]


def test_refusals_that_need_no_device(urlib):
    """Every check comes before the context is looked at: a stand-in context is enough, the addresses are numbers and none is dereferenced.
    The host twin has the same refusals but for the context."""
    from unclerenderer_amd import lib
    stand_in = C.create_string_buffer(4096)
    w, h, base, taps = 64, 32, 16, 4
    ok = dict(ctx=C.addressof(stand_in), src=0x100000, src_bytes=4 * w * h, w=w, h=h, base=base, taps=taps, dst=0x300000, dst_bytes=48 * base * base)

    def device(**kw):
        a = dict(ok, **kw)
        rc = urlib.ur_env_panorama(a["ctx"], a["src"], a["src_bytes"], a["w"], a["h"], a["base"], a["taps"], a["dst"], a["dst_bytes"])
        return rc, urlib.ur_last_error().decode()

    def host_twin(**kw):
        a = dict(ok, **kw)
        return urlib.ur_host_env_panorama(a["src"], a["src_bytes"], a["w"], a["h"], a["base"], a["taps"], a["dst"], a["dst_bytes"])

    def refused(text, **kw):
        rc, said = device(**kw)
        assert rc == lib.UR_EINVAL and text in said, (text, kw, rc, said)
        if "ctx" not in kw:
            assert host_twin(**kw) == lib.UR_EINVAL, kw

    refused("null context", ctx=None)
    refused("null source or destination", src=None)
    refused("null source or destination", dst=None)
    for bad in (0, 16385, 1 << 31):
        refused(f"a panorama of {bad} x {h}", w=bad)
    for bad in (0, 8193, 1 << 31):
        refused(f"a panorama of {w} x {bad}", h=bad)
    for b in (0, 3, 12, 24, 4096, 1 << 31):
        refused(f"base size {b}", base=b)
    for k in (0, 3, 6, 12, 32, 64, 1 << 31):
        refused(f"{k} taps a side", taps=k)
    refused("source bytes", src_bytes=ok["src_bytes"] - 4)
    refused("source bytes", src_bytes=ok["src_bytes"] + 4)
    refused("source bytes", w=w + 1)  # another panorama's size
    refused("destination bytes", dst_bytes=ok["dst_bytes"] - 8)
    refused("destination bytes", dst_bytes=ok["dst_bytes"] + 8)
    refused("destination bytes", base=32)  # another cube's size
    for off in (1, 2, 3):
        refused("source not 4-byte aligned", src=ok["src"] + off)
    for off in (4, 8, 12):
        refused("destination not 16-byte aligned", dst=ok["dst"] + off)
    refused("source and destination overlap", dst=ok["src"] + ok["src_bytes"] - 16)  # the destination begins in the source's last bytes
    refused("source and destination overlap", src=ok["dst"] + ok["dst_bytes"] - 4)   # the source begins in the destination's last bytes
    refused("source and destination overlap", src=ok["dst"])
    assert urlib.ur_host_env_panorama_taps(0, 1, 1) == 0 and urlib.ur_host_env_panorama_taps(1, 1, 3) == 0 and urlib.ur_host_env_panorama_taps(1, 8193, 1) == 0


def test_python_functions_refuse(urlib, monkeypatch):
    from unclerenderer_amd import environment, hostmath, hotpath
    from unclerenderer_amd.hotpath import tensors

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

    monkeypatch.setattr(tensors.torch, "Tensor", T)

    class NoDevice(hotpath.HotPath):
        def __init__(self):
            self._L, self._ctx, self.device = urlib, None, 0
    hp = NoDevice()
    for w, h, base, taps in ((0, 4, 8, 1), (16385, 4, 8, 1), (8, 0, 8, 1), (8, 8193, 8, 1), (8, 4, 24, 1), (8, 4, 4096, 1), (8, 4, 8, 3), (8, 4, 8, 32), (8, 4, 8, 0)):
        with pytest.raises(ValueError, match="no panorama build"):
            environment.panorama_to_cube(hp, T(0x1000, 4 * w * h), w, h, base, taps)
    with pytest.raises(ValueError, match="no panorama build"):
        environment.panorama_to_cube(hp, T(0x1000, 128), 8, 4, 24)  # (the recommendation refuses the sizes)
    with pytest.raises(ValueError, match="is 128 bytes, the source has 124"):
        environment.panorama_to_cube(hp, T(0x1000, 124), 8, 4, 16)
    with pytest.raises(ValueError, match="the source has 100"):
        environment.panorama_to_cube(hp, bytes(100), 8, 4, 16)  # refused before any upload
    with pytest.raises(ValueError, match="the source has 100"):
        environment.bake_panorama(hp, bytes(100), 8, 4, 16, 64)
    with pytest.raises(ValueError, match="is 12288 bytes, out has 12280"):
        environment.panorama_to_cube(hp, T(0x1000, 128), 8, 4, 16, out=T(0x4000, 12280))
    with pytest.raises(ValueError, match="ur_host_env_panorama failed"):
        hostmath.env_panorama(np.zeros(100, np.uint8), 8, 4, 16)
    with pytest.raises(ValueError, match="ur_host_env_panorama failed"):
        hostmath.env_panorama(np.zeros(128, np.uint8), 8, 4, 16, 5)
    with pytest.raises(ValueError, match="no panorama build"):
        hostmath.env_panorama(np.zeros(128, np.uint8), 8, 4, 24)
    cube = hostmath.env_panorama(np.zeros(128, np.uint8), 8, 4, 16)
    assert cube.shape == (6, 16, 16, 4) and cube.dtype == np.uint16 and (cube[..., :3] == 0).all() and (cube[..., 3] == 0x3C00).all()


def test_new_kernel_uses_no_scratch_and_the_old_ones_are_as_they_were(urlib, tmp_path):
    """The code objects' metadata notes. The new kernel has no scratch and spills nothing (DESIGN.md 3.21 records the counts). Every kernel
    of the commit before (tests/golden/kernel_metadata_before_env_panorama.json: private segment, SGPRs, spilled SGPRs, VGPRs, spilled
    VGPRs, recorded from that commit's library) is still there with the same figures."""
    from tests.code_objects import library_kernels
    kernels = library_kernels(tmp_path)
    new = {k: v for k, v in kernels.items() if re.search(r"panorama_\w+_kernel", k)}
    assert len(new) == 1, sorted(new)
    assert not [k for k in new if re.search(r"env_bake_\w+_kernel|env_cube_\w+_kernel", k)]
    for name, meta in new.items():
        print(name, meta)
        assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0 and meta["sgpr_spill_count"] == 0, (name, meta)
        assert meta["vgpr_count"] <= 64, (name, meta)  # eight waves a SIMD
    before = json.loads((ROOT / "tests" / "golden" / "kernel_metadata_before_env_panorama.json").read_text())
    keys = ("private_segment_fixed_size", "sgpr_count", "sgpr_spill_count", "vgpr_count", "vgpr_spill_count")
    assert len(before) == 142 and not set(before) & set(new) and set(kernels) == set(before) | set(new)
    moved = {k: (v, [kernels.get(k, {}).get(f) for f in keys]) for k, v in before.items() if [kernels.get(k, {}).get(f) for f in keys] != v}
    assert not moved, moved
