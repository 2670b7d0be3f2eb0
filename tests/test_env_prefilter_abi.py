"""The environment prefilter's ABI without a GPU (include/ur_env_prefilter.h): the header against a compiled probe, the
symbols declared, exported and bound, every refusal of both entry points and of the table function - decided before a device is needed -
the Python wrappers' refusals, the host unit built by the plain host compiler, the host code and the launches' items under ASan / UBSan in
a stand-alone program (tests/cpp/env_prefilter_main.cpp), and the kernels' resources from the built library's metadata."""
import ctypes as C
import json
import re
import subprocess

import numpy as np
import pytest

from tests import env_prefilter_ref as P
from tests.test_bcn_abi import ROOT, _cxx

CSRC = ROOT / "unclerenderer_amd" / "csrc"
HOST_UNITS = [str(CSRC / n) for n in ("env_prefilter_host.cpp", "env_cube_host.cpp", "env_cube_stage.cpp", "lighting_plan.cpp")]
NEW = {"ur_env_prefilter_table_bytes": "ur_env_prefilter.h", "ur_env_prefilter_scratch_bytes": "ur_env_prefilter.h", "ur_env_prefilter": "ur_env_prefilter.h",
       "ur_host_env_prefilter_table": "ur_host.h", "ur_host_env_prefilter": "ur_host.h"}


def test_header_against_a_compiled_probe(tmp_path):
    from unclerenderer_amd import lib
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include "ur_env_prefilter.h"\nint main(void) { printf("%u %u %u %u %zu %zu %zu %zu\\n", UR_ENV_PREFILTER_MAX_BASE_SIZE, '
                   "UR_ENV_PREFILTER_MIN_SAMPLES, UR_ENV_PREFILTER_MAX_SAMPLES, UR_ENV_PREFILTER_MAX_STREAM_OPS, ur_env_prefilter_table_bytes(256u, 1024u), "
                   "ur_env_prefilter_table_bytes(1u, 16u), ur_env_prefilter_scratch_bytes(4u), ur_env_prefilter_scratch_bytes(3u)); "
                   "int (*run)(ur_ctx*, const void*, size_t, uint32_t, uint32_t, const void*, size_t, void*, size_t, void*, size_t) = ur_env_prefilter; "
                   "(void)run; return 0; }\n")
    stub = tmp_path / "stub.c"  # (the probe takes the entry point's address: the host units have the size functions, a stub stands for the device call)
    stub.write_text('#include "ur_env_prefilter.h"\nint ur_env_prefilter(ur_ctx* c, const void* s, size_t n, uint32_t b, uint32_t k, const void* t, size_t tn, void* d, '
                    "size_t dn, void* x, size_t xn)\n{ (void)c; (void)s; (void)n; (void)b; (void)k; (void)t; (void)tn; (void)d; (void)dn; (void)x; (void)xn; return 0; }\n")
    so, exe = tmp_path / "libhost.so", tmp_path / "probe"
    cc = _cxx().replace("g++", "gcc").replace("c++", "cc")
    subprocess.run([_cxx(), "-std=c++17", "-shared", "-fPIC"] + HOST_UNITS + ["-o", str(so)], check=True)
    subprocess.run([cc, "-std=c99", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}", str(src), str(stub), str(so), f"-Wl,-rpath,{tmp_path}", "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    # 256: nine levels, 16 * 9 + 16 * 1024 * 8. 4: payload 6 * 21 * 8 bytes, bordered faces 6 * (36 + 16 + 9) * 8 bytes
    assert got == [2048, 16, 4096, 15, 144 + 131072, 16, 1008 + 2928, 0]
    assert got[:4] == [lib.UR_ENV_PREFILTER_MAX_BASE_SIZE, lib.UR_ENV_PREFILTER_MIN_SAMPLES, lib.UR_ENV_PREFILTER_MAX_SAMPLES, lib.UR_ENV_PREFILTER_MAX_STREAM_OPS]
    # the bound on the launches, whatever the base: top, a pyramid launch a level below the top, two staging launches, the filter
    assert max(1 + (P.levels_of(b) - 1) + 2 + 1 for b in (2 ** i for i in range(12))) == lib.UR_ENV_PREFILTER_MAX_STREAM_OPS


def test_symbols_declared_exported_and_bound(urlib):
    from unclerenderer_amd import assets, build, hostmath, hotpath, lib
    strip = lambda text: re.sub(r"/\*.*?\*/", "", text, flags=re.S)  # noqa: E731
    for name, header in NEW.items():
        assert re.search(r"\b%s\s*\(" % name, strip((ROOT / "include" / header).read_text())), name
        assert name in lib.SIGNATURES and getattr(urlib, name) is not None
    assert callable(hotpath.HotPath.prefilter_env_cube) and callable(hotpath.HotPath.bake_env_cube)
    assert callable(hostmath.env_prefilter_table) and callable(hostmath.env_prefilter) and callable(assets.load_env_cube_top_level)
    for header in ("ur_frame.h", "ur_hotpath.h"):  # nothing is wired into the frame, and the hot path's header has no new entry point
        assert "env_prefilter" not in strip((ROOT / "include" / header).read_text())
    flags = dict(build.SOURCES)
    assert flags["env_prefilter.hip"] == build.EXACT and "-ffp-contract=off" in flags["env_prefilter_host.cpp"]
    # one sampler for the new unit, in a header; the device unit names no transcendental function
    device = re.sub(r"//.*", "", (CSRC / "env_prefilter.hip").read_text() + (CSRC / "env_prefilter_rule.h").read_text() + (CSRC / "cube_sample.h").read_text())
    assert not re.search(r"\b(sinf?|cosf?|log2f?|powf?|expf?|__sinf|__cosf)\s*\(", device)


def test_the_host_unit_builds_with_the_plain_compiler_and_builds_the_same(tmp_path, urlib):
    so = tmp_path / "libenv_prefilter_host.so"
    subprocess.run([_cxx(), "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC"] + HOST_UNITS + ["-o", str(so)], check=True)
    from unclerenderer_amd import hostmath
    plain = C.CDLL(str(so))
    for base, samples in ((8, 64), (16, 16)):
        top = P.random_cube(base + samples, base)
        assert np.array_equal(hostmath.env_prefilter_table(base, samples), hostmath.env_prefilter_table(base, samples, library=plain))
        assert np.array_equal(hostmath.env_prefilter(top, base, samples), hostmath.env_prefilter(top, base, samples, library=plain))


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    """tests/cpp/env_prefilter_main.cpp with the host units, built once with -fsanitize=address,undefined: its own main, no Python, no device."""
    exe = tmp_path_factory.mktemp("env_prefilter_sanitize") / "env_prefilter_main"
    subprocess.run([_cxx(), "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    str(ROOT / "tests" / "cpp" / "env_prefilter_main.cpp")] + HOST_UNITS + ["-o", str(exe)], check=True)
    return exe


def test_closed_form_layout_and_half_conversions(sanitized):
    """The closed forms of the rule against ur::cube_layout for every base 1 .. 2048, and the host's fp16 conversions over every half and
    every rounding boundary."""
    r = subprocess.run([str(sanitized), "layout"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "layout ok", (r.stdout[-1000:], r.stderr[-2000:])


@pytest.mark.parametrize("base,samples", [(1, 16), (2, 16), (4, 64), (16, 32), (32, 128), (8, 4096)])
def test_host_build_and_the_items_under_asan_and_ubsan(sanitized, tmp_path, base, samples):
    """The table and the host build into heap buffers of exactly their sizes, then the device's launches item by item on the host (the
    functions the kernels call), descending, into buffers that arrive as 0xFF: the same bytes, no access outside a buffer."""
    from unclerenderer_amd import hostmath
    top = P.random_cube(11 * base + samples, base)
    blob = tmp_path / "cube.bin"
    blob.write_bytes(np.uint32([base, samples, 0, 0]).tobytes() + top.tobytes())
    r = subprocess.run([str(sanitized), "build", str(blob)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
    want = hostmath.env_prefilter(top, base, samples)
    assert r.stdout.split() == ["0", str(int(want.view(np.uint8).sum(dtype=np.uint64)))]


def test_refusals_that_need_no_device(urlib):
    """Every check comes before the context is looked at: a stand-in context is enough, the addresses are numbers and none is dereferenced.
    The host twin has the same refusals but for the context and the scratch."""
    from unclerenderer_amd import lib
    stand_in = C.create_string_buffer(4096)
    base, samples = 16, 64
    table, scratch = int(urlib.ur_env_prefilter_table_bytes(base, samples)), int(urlib.ur_env_prefilter_scratch_bytes(base))
    dst = int(urlib.ur_env_cube_source_bytes(lib.UR_ENV_SOURCE_RGBA16F, base, 5))
    assert (table, dst) == (16 * 5 + 16 * 64 * 4, 6 * 341 * 8) and scratch > dst
    ok = dict(ctx=C.addressof(stand_in), src=0x100000, src_bytes=48 * base * base, base=base, samples=samples, table=0x200000, table_bytes=table, dst=0x300000,
              dst_bytes=dst, scratch=0x400000, scratch_bytes=scratch)

    def device(**kw):
        a = dict(ok, **kw)
        rc = urlib.ur_env_prefilter(a["ctx"], a["src"], a["src_bytes"], a["base"], a["samples"], a["table"], a["table_bytes"], a["dst"], a["dst_bytes"], a["scratch"],
                                    a["scratch_bytes"])
        return rc, urlib.ur_last_error().decode()

    def host_twin(**kw):
        a = dict(ok, **kw)
        return urlib.ur_host_env_prefilter(a["src"], a["src_bytes"], a["base"], a["samples"], a["table"], a["table_bytes"], a["dst"], a["dst_bytes"])

    def refused(text, **kw):
        rc, said = device(**kw)
        assert rc == lib.UR_EINVAL and text in said, (text, kw, rc, said)
        if "ctx" not in kw and not any(k.startswith("scratch") for k in kw) and "scratch" not in text:
            assert host_twin(**kw) == lib.UR_EINVAL, kw

    refused("null context", ctx=None)
    for name in ("src", "table", "dst", "scratch"):
        refused("null source, table, destination or scratch", **{name: None})
    for b in (0, 3, 12, 24, 4096, 1 << 31):
        refused(f"base size {b}", base=b)
    for s in (0, 8, 15, 48, 1000, 8192):
        refused(f"sample count {s}", samples=s)
    refused("source bytes", src_bytes=ok["src_bytes"] - 8)
    refused("source bytes", src_bytes=ok["src_bytes"] + 8)
    refused("source bytes", base=32)  # another cube's size
    refused("destination bytes", dst_bytes=dst - 8)
    refused("destination bytes", dst_bytes=dst + 8)
    refused("destination bytes", dst_bytes=int(urlib.ur_env_cube_source_bytes(lib.UR_ENV_SOURCE_RGBA16F, base, 4)))  # a chain that is not full
    refused("table bytes", table_bytes=table - 16)
    refused("table bytes", samples=128)  # the table of fewer samples is short
    refused("scratch bytes", scratch_bytes=scratch - 8)
    refused("scratch bytes", scratch_bytes=0)
    for name, word in (("src", "source"), ("table", "table"), ("dst", "destination"), ("scratch", "scratch")):
        refused(f"{word} not 16-byte aligned", **{name: ok[name] + 8})
    sizes = dict(src=ok["src_bytes"], table=table, dst=dst, scratch=scratch)
    words = dict(src="source", table="table", dst="destination", scratch="scratch")
    order = ("src", "table", "dst", "scratch")
    for i, a in enumerate(order):
        for b in order[i + 1:]:
            text = f"{words[a]} and {words[b]} overlap"
            refused(text, **{b: ok[a] + sizes[a] - 16})  # b begins in a's last bytes
            refused(text, **{a: ok[b] + sizes[b] - 16})  # a begins in b's last bytes
    # the table function
    out = np.zeros(table + 16, np.uint8)
    at = C.c_void_p(out.ctypes.data)
    assert urlib.ur_host_env_prefilter_table(base, samples, None, table) == lib.UR_EINVAL
    assert urlib.ur_host_env_prefilter_table(base, samples, at, table - 1) == lib.UR_EINVAL
    assert urlib.ur_host_env_prefilter_table(24, samples, at, table) == lib.UR_EINVAL
    assert urlib.ur_host_env_prefilter_table(base, 48, at, table) == lib.UR_EINVAL
    out[:] = 0xAB
    assert urlib.ur_host_env_prefilter_table(base, samples, at, table) == 0 and (out[table:] == 0xAB).all() and out[:4].view(np.float32)[0] == 1.0
    for b, s in ((0, 64), (4096, 64), (24, 64), (16, 8), (16, 8192), (16, 100)):
        assert urlib.ur_env_prefilter_table_bytes(b, s) == 0
    assert urlib.ur_env_prefilter_scratch_bytes(0) == 0 and urlib.ur_env_prefilter_scratch_bytes(4096) == 0 and urlib.ur_env_prefilter_scratch_bytes(48) == 0


def test_python_wrappers_refuse(urlib, monkeypatch):
    from unclerenderer_amd import hostmath, hotpath

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
    for base, samples in ((24, 64), (0, 64), (4096, 64), (16, 8), (16, 100)):
        with pytest.raises(ValueError, match="no prefilter"):
            NoDevice().prefilter_env_cube(T(0x1000, 48 * base * base), base, samples)
        with pytest.raises(ValueError, match="no prefilter table"):
            hostmath.env_prefilter_table(base, samples)
    with pytest.raises(ValueError, match="is 12288 bytes, the source has 12280"):
        NoDevice().prefilter_env_cube(T(0x1000, 12280), 16, 64)
    with pytest.raises(ValueError, match="the source has 100"):
        NoDevice().prefilter_env_cube(bytes(100), 16, 64)  # refused before any upload
    with pytest.raises(ValueError, match="the source has 100"):
        NoDevice().bake_env_cube(bytes(100), 16, 64)
    with pytest.raises(ValueError, match="ur_host_env_prefilter failed"):
        hostmath.env_prefilter(np.zeros(100, np.uint8), 16, 64)
    with pytest.raises(ValueError, match="ur_host_env_prefilter failed"):
        hostmath.env_prefilter(np.zeros(48 * 16 * 16, np.uint8), 16, 64, table=hostmath.env_prefilter_table(16, 32))  # a short table
    chain = hostmath.env_prefilter(np.zeros(48 * 16 * 16, np.uint8), 16, 64)
    assert chain.shape == (6 * 341, 4) and chain.dtype == np.uint16 and (chain[:, :3] == 0).all() and (chain[:, 3] == 0x3C00).all()


def test_top_level_of_the_shipped_cube():
    from unclerenderer_amd import assets
    path = ROOT / "tests" / "golden" / "assets" / "output_pmrem.dds"
    top, base = assets.load_env_cube_top_level(path)
    cube, base2, mips, _ = assets.load_env_cube_dds(path)
    per_face = cube.shape[0] // 6
    assert base == base2 == 256 and top.shape == (6, 256, 256, 4) and top.dtype == np.uint16
    for f in range(6):
        assert np.array_equal(top[f].reshape(-1, 4), cube[f * per_face:f * per_face + base * base])


def test_new_kernels_use_no_scratch_and_the_old_ones_are_as_they_were(urlib, tmp_path):
    """The code objects' metadata notes. The three new kernels have no scratch and spill nothing (DESIGN.md 3.20 records the counts). Every
    kernel of the commit before the prefilter (tests/golden/kernel_metadata_before_env_prefilter.json: private segment, SGPRs, spilled
    SGPRs, VGPRs, spilled VGPRs, recorded from that commit's library) is still there with the same figures."""
    from tests.code_objects import library_kernels
    kernels = library_kernels(tmp_path)
    new = {k: v for k, v in kernels.items() if re.search(r"env_bake_\w+_kernel", k)}
    assert len(new) == 3, sorted(new)  # top, down, filter
    for name, meta in new.items():
        print(name, meta)
        assert meta["private_segment_fixed_size"] == 0 and meta["vgpr_spill_count"] == 0 and meta["sgpr_spill_count"] == 0, (name, meta)
        assert meta["vgpr_count"] <= 64, (name, meta)  # eight waves a SIMD
    before = json.loads((ROOT / "tests" / "golden" / "kernel_metadata_before_env_prefilter.json").read_text())
    keys = ("private_segment_fixed_size", "sgpr_count", "sgpr_spill_count", "vgpr_count", "vgpr_spill_count")
    assert len(before) == 139 and not set(before) & set(new)
    moved = {k: (v, [kernels.get(k, {}).get(f) for f in keys]) for k, v in before.items() if [kernels.get(k, {}).get(f) for f in keys] != v}
    assert not moved, moved
