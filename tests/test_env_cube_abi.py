"""The environment cube build's ABI without a GPU (include/ur_env_cube.h): the header against a compiled probe, the symbols
declared, exported and bound, every refusal of both entry points - decided before a device is needed - the Python routing, the host unit
built by the plain host compiler, the host code under ASan / UBSan in a stand-alone program (tests/cpp/env_cube_main.cpp), and the
kernels' resources from the built library's metadata."""
import ctypes as C
import json
import re
import subprocess

import numpy as np
import pytest

from tests import env_cube_ref as R
from tests.test_bcn_abi import ROOT, _cxx

CSRC = ROOT / "unclerenderer_amd" / "csrc"
HOST_UNITS = [str(CSRC / "env_cube_host.cpp"), str(CSRC / "env_cube_stage.cpp"), str(CSRC / "lighting_plan.cpp")]
NEW = {"ur_env_cube_source_bytes": "ur_env_cube.h", "ur_env_cube_build": "ur_env_cube.h", "ur_host_env_cube_build": "ur_host.h"}


def test_header_against_a_compiled_probe(tmp_path):
    from unclerenderer_amd import lib
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include "ur_env_cube.h"\nint main(void) { printf("%u %u %u %u %u %zu\\n", UR_ENV_SOURCE_RGBA16F, UR_ENV_SOURCE_BC6H_UF16, '
                   "UR_ENV_SOURCE_BC6H_SF16, UR_ENV_CUBE_BUILD_MAX_STREAM_OPS, UR_ENV_CUBE_MAX_BASE_SIZE, sizeof(ur_half4)); "
                   "int (*build)(ur_ctx*, const void*, size_t, uint32_t, uint32_t, uint32_t, ur_half4*, size_t, uint32_t*) = ur_env_cube_build; "
                   "size_t (*bytes)(uint32_t, uint32_t, uint32_t) = ur_env_cube_source_bytes; (void)build; return bytes(95u, 4u, 3u) == 288 ? 0 : 1; }\n")
    exe = tmp_path / "probe"
    so = tmp_path / "libhost.so"  # (the probe takes the functions' addresses: it links against the host unit, which has one of them, and a stub)
    stub = tmp_path / "stub.c"
    stub.write_text('#include "ur_env_cube.h"\nint ur_env_cube_build(ur_ctx* c, const void* s, size_t n, uint32_t f, uint32_t b, uint32_t m, ur_half4* d, size_t t, uint32_t* i)\n'
                    "{ (void)c; (void)s; (void)n; (void)f; (void)b; (void)m; (void)d; (void)t; (void)i; return 0; }\n")
    cc = _cxx().replace("g++", "gcc").replace("c++", "cc")
    subprocess.run([_cxx(), "-std=c++17", "-shared", "-fPIC"] + HOST_UNITS + ["-o", str(so)], check=True)
    subprocess.run([cc, "-std=c99", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}", str(src), str(stub), str(so), f"-Wl,-rpath,{tmp_path}", "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [10, 95, 96, 3, 16384, 8]
    assert got[:5] == [lib.UR_ENV_SOURCE_RGBA16F, lib.UR_ENV_SOURCE_BC6H_UF16, lib.UR_ENV_SOURCE_BC6H_SF16, lib.UR_ENV_CUBE_BUILD_MAX_STREAM_OPS, lib.UR_ENV_CUBE_MAX_BASE_SIZE]


def test_symbols_declared_exported_and_bound(urlib):
    from unclerenderer_amd import assets, hostmath, hotpath, lib
    strip = lambda text: re.sub(r"/\*.*?\*/", "", text, flags=re.S)  # noqa: E731
    for name, header in NEW.items():
        assert re.search(r"\b%s\s*\(" % name, strip((ROOT / "include" / header).read_text())), name
        assert name in lib.SIGNATURES and getattr(urlib, name) is not None
    assert callable(hotpath.HotPath.build_env_cube) and callable(hostmath.env_cube_build) and callable(assets.load_env_cube_dds_source)
    assert "env_cube_build" not in strip((ROOT / "include" / "ur_frame.h").read_text())  # nothing is wired into the frame
    from unclerenderer_amd import build
    assert {"env_cube_build.hip", "env_cube_host.cpp"} <= {s for s, _ in build.SOURCES}
    # one decoder: dds.cpp holds no copy of it
    text = (CSRC / "dds.cpp").read_text()
    assert '#include "bc6h_decode.h"' in text and "kPartition2" not in text and "BitReader" not in text and "finish_unquantize" not in text


def test_the_host_unit_builds_with_the_plain_compiler_and_builds_the_same(tmp_path, urlib):
    so = tmp_path / "libenv_cube_host.so"
    subprocess.run([_cxx(), "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC"] + HOST_UNITS + ["-o", str(so)], check=True)
    subprocess.run([_cxx(), "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-c", str(CSRC / "dds.cpp"), "-o", str(tmp_path / "dds.o")], check=True)
    from unclerenderer_amd import hostmath
    plain = C.CDLL(str(so))
    for fmt, base, mips in ((R.SF16, 7, 3), (R.UF16, 12, 1), (R.RGBA16F, 5, 3)):
        payload = R.random_payload(base, fmt, base, mips)
        ours, bad = hostmath.env_cube_build(payload, fmt, base, mips)
        theirs, bad2 = hostmath.env_cube_build(payload, fmt, base, mips, library=plain)
        want, bad3 = R.build(urlib, payload, fmt, base, mips)
        assert bad == bad2 == bad3 and np.array_equal(ours, want) and np.array_equal(theirs, want)


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    """tests/cpp/env_cube_main.cpp with the host units, built once with -fsanitize=address,undefined: its own main, no Python, no device."""
    exe = tmp_path_factory.mktemp("env_cube_sanitize") / "env_cube_main"
    subprocess.run([_cxx(), "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    str(ROOT / "tests" / "cpp" / "env_cube_main.cpp")] + HOST_UNITS + ["-o", str(exe)], check=True)
    return exe


def test_integer_border_rule_is_the_staging_rule(sanitized):
    """csrc/env_cube_rule.h's border_source against resolve_border (doubles) through ur::stage_env_cube_host: every edge 1..64, and 256."""
    r = subprocess.run([str(sanitized), "rule"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "rule ok", (r.stdout[-1000:], r.stderr[-2000:])


@pytest.mark.parametrize("fmt,base,mips", [(R.SF16, 1, 1), (R.SF16, 6, 3), (R.UF16, 33, 6), (R.RGBA16F, 5, 3), (R.SF16, 64, 7)])
def test_host_build_and_the_items_under_asan_and_ubsan(sanitized, urlib, tmp_path, fmt, base, mips):
    """The host build into heap buffers of exactly their sizes, then the device's three launches item by item on the host (the functions
    the kernels call, one item a lane): the same bytes, no access outside a buffer, and the host build's bytes are the restatement's."""
    payload = R.random_payload(7 * base + fmt, fmt, base, mips)
    blob = tmp_path / "cube.bin"
    blob.write_bytes(np.uint32([fmt, base, mips, 0]).tobytes() + payload.tobytes())
    r = subprocess.run([str(sanitized), "build", str(blob)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
    from unclerenderer_amd import hostmath
    want, bad = (R.build(urlib, payload, fmt, base, mips) if base <= 33 else hostmath.env_cube_build(payload, fmt, base, mips))
    assert r.stdout.split() == ["0", str(int(want.view(np.uint8).sum(dtype=np.uint64))), str(bad)]


def test_refusals_that_need_no_device(urlib):
    """Every check comes before the context is looked at: a stand-in context is enough, the addresses are numbers and none is dereferenced.
    The host twin has the same refusals but for the context."""
    from unclerenderer_amd import lib
    stand_in = C.create_string_buffer(4096)
    fmt, base, mips = lib.UR_ENV_SOURCE_BC6H_SF16, 16, 5
    need, texels = int(urlib.ur_env_cube_source_bytes(fmt, base, mips)), int(urlib.ur_env_cube_texels(base, mips))
    ok = dict(ctx=C.addressof(stand_in), src=0x100000, src_bytes=need, format=fmt, base=base, mips=mips, dst=0x200000, dst_texels=texels, info=0x300000)

    def device(**kw):
        a = dict(ok, **kw)
        rc = urlib.ur_env_cube_build(a["ctx"], a["src"], a["src_bytes"], a["format"], a["base"], a["mips"], a["dst"], a["dst_texels"], a["info"])
        return rc, urlib.ur_last_error().decode()

    def host_twin(**kw):
        a = dict(ok, **kw)
        return urlib.ur_host_env_cube_build(a["src"], a["src_bytes"], a["format"], a["base"], a["mips"], a["dst"], a["dst_texels"], a["info"])

    def refused(text, **kw):
        rc, said = device(**kw)
        assert rc == lib.UR_EINVAL and text in said, (text, kw, rc, said)
        if "ctx" not in kw:
            assert host_twin(**kw) == lib.UR_EINVAL, kw

    refused("null context", ctx=None)
    refused("null source or destination", src=None)
    refused("null source or destination", dst=None)
    for f in (0, 11, 71, 94, 97, 98):
        refused(f"source format {f}", format=f, src_bytes=0)
    refused("no cube", base=0, src_bytes=0, dst_texels=0)
    refused("no cube", mips=0, src_bytes=0, dst_texels=0)
    refused("no cube", mips=17, src_bytes=0, dst_texels=0)
    refused("no cube", base=16385, mips=1, src_bytes=int(urlib.ur_env_cube_source_bytes(fmt, 16385, 1)), dst_texels=int(urlib.ur_env_cube_texels(16385, 1)))
    refused("source bytes", src_bytes=need - 16)
    refused("source bytes", src_bytes=need + 16)
    refused("source bytes", format=lib.UR_ENV_SOURCE_RGBA16F)  # the same cube in another format is another size
    refused("destination texels", dst_texels=texels - 1)
    refused("destination texels", dst_texels=texels + 1)
    refused("destination texels", dst_texels=int(urlib.ur_env_cube_texels(base, mips - 1)), mips=mips, src_bytes=need)
    refused("source not 16-byte aligned", src=ok["src"] + 8)
    refused("destination not 16-byte aligned", dst=ok["dst"] + 8)
    refused("info not 4-byte aligned", info=ok["info"] + 2)
    refused("source and destination overlap", dst=ok["src"] + need - 16)
    refused("source and destination overlap", src=ok["dst"] + 8 * texels - 16)
    refused("source and info overlap", info=ok["src"] + need - 4)
    refused("destination and info overlap", info=ok["dst"])
    refused("destination and info overlap", info=ok["dst"] + 8 * texels - 4)


def test_python_routing(urlib, monkeypatch):
    from unclerenderer_amd import hostmath, hotpath, lib

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

    monkeypatch.setattr(hotpath.torch, "Tensor", T)

    class NoDevice(hotpath.HotPath):
        def __init__(self):
            self._L, self._ctx, self.device = urlib, None, 0
    with pytest.raises(ValueError, match="no cube source"):
        NoDevice().build_env_cube(T(0x1000, 288), 97, 4, 3)
    with pytest.raises(ValueError, match="is 288 bytes, the payload has 272"):
        NoDevice().build_env_cube(T(0x1000, 272), lib.UR_ENV_SOURCE_BC6H_UF16, 4, 3)
    with pytest.raises(ValueError, match="the payload has 100"):
        NoDevice().build_env_cube(bytes(100), lib.UR_ENV_SOURCE_BC6H_UF16, 4, 3)  # refused before any upload
    with pytest.raises(ValueError, match="ur_host_env_cube_build failed"):
        hostmath.env_cube_build(np.zeros(272, np.uint8), lib.UR_ENV_SOURCE_BC6H_UF16, 4, 3)
    cube, bad = hostmath.env_cube_build(bytes(288), lib.UR_ENV_SOURCE_BC6H_UF16, 4, 3)  # all-zero blocks are mode 1 with zero endpoints
    assert bad == 0 and cube.shape == (int(urlib.ur_env_cube_texels(4, 3)), 4) and cube.dtype == np.uint16


def test_new_kernels_use_no_scratch_and_the_old_ones_are_as_they_were(urlib, tmp_path):
    """The code objects' metadata notes. The five new kernels have no scratch and spill nothing (DESIGN.md 3.19 records the counts). Every
    kernel of the commit before the environment cube build (tests/golden/kernel_metadata_before_env_cube.json: private segment, SGPRs,
    spilled SGPRs, VGPRs, spilled VGPRs, recorded from that commit's library) is still there with the same figures: the new unit is a
    translation unit of its own and moved nobody's registers. A change that means to move a kernel's figures records them anew."""
    from tests.code_objects import library_kernels
    kernels = library_kernels(tmp_path)
    new = {k: v for k, v in kernels.items() if re.search(r"env_cube_\w+_kernel", k)}
    assert len(new) == 5, sorted(new)  # decode in its three formats, border, pairs
    for name, meta in new.items():
        print(name, meta)
        assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0 and meta["sgpr_spill_count"] == 0, (name, meta)
        assert meta["vgpr_count"] <= 64, (name, meta)  # eight waves a SIMD
    before = json.loads((ROOT / "tests" / "golden" / "kernel_metadata_before_env_cube.json").read_text())
    keys = ("private_segment_fixed_size", "sgpr_count", "sgpr_spill_count", "vgpr_count", "vgpr_spill_count")
    assert len(before) == 134 and not set(before) & set(new)
    moved = {k: (v, [kernels.get(k, {}).get(f) for f in keys]) for k, v in before.items() if [kernels.get(k, {}).get(f) for f in keys] != v}
    assert not moved, moved
