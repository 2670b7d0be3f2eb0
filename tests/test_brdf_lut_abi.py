"""The ABI of the BRDF LUT without a GPU (include/ur_brdf_lut.h): the header against a compiled probe, every refusal of
ur_brdf_lut, ur_host_brdf_lut and ur_host_brdf_lut_table - decided before a device is needed - and the Python functions' refusals.
The symbols, the host units, the sanitizer program and the kernel's metadata are held by tests/test_env_sky_abi.py with the capture's."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from tests.test_bcn_abi import ROOT, _cxx
from tests.test_env_sky_abi import HOST_UNITS


def test_header_against_a_compiled_probe(tmp_path):
    from unclerenderer_amd import lib
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include "ur_brdf_lut.h"\n#include "ur_host.h"\n'
                   'int main(void) { printf("%u %u %u %u %u %zu %zu %zu %zu %zu\\n", UR_BRDF_LUT_MAX_WIDTH, UR_BRDF_LUT_MAX_HEIGHT, UR_BRDF_LUT_MIN_SAMPLES, '
                   "UR_BRDF_LUT_MAX_SAMPLES, UR_BRDF_LUT_MAX_STREAM_OPS, ur_brdf_lut_table_bytes(32u, 1024u), ur_brdf_lut_table_bytes(256u, 4096u), "
                   "ur_brdf_lut_table_bytes(0u, 64u), ur_brdf_lut_table_bytes(257u, 64u), ur_brdf_lut_table_bytes(32u, 48u)); "
                   "int (*run)(ur_ctx*, uint32_t, uint32_t, uint32_t, const void*, size_t, void*, size_t) = ur_brdf_lut; "
                   "int (*twin)(uint32_t, uint32_t, uint32_t, const void*, size_t, void*, size_t) = ur_host_brdf_lut; "
                   "int (*table)(uint32_t, uint32_t, void*, size_t) = ur_host_brdf_lut_table; (void)run; (void)twin; (void)table; return 0; }\n")
    stub = tmp_path / "stub.c"  # (the probe takes the entry point's address: the host units have the rest, a stub stands for the device calls)
    stub.write_text('#include "ur_brdf_lut.h"\n#include "ur_env_sky.h"\n'
                    "int ur_brdf_lut(ur_ctx* c, uint32_t w, uint32_t h, uint32_t s, const void* t, size_t tn, void* d, size_t dn)\n"
                    "{ (void)c; (void)w; (void)h; (void)s; (void)t; (void)tn; (void)d; (void)dn; return 0; }\n")
    so, exe = tmp_path / "libhost.so", tmp_path / "probe"
    cc = _cxx().replace("g++", "gcc").replace("c++", "cc")
    subprocess.run([_cxx(), "-std=c++17", "-shared", "-fPIC"] + HOST_UNITS + ["-o", str(so)], check=True)
    subprocess.run([cc, "-std=c99", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}", str(src), str(stub), str(so), f"-Wl,-rpath,{tmp_path}", "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [1024, 256, 16, 4096, 1, 16 * 32 * 1024, 16 * 256 * 4096, 0, 0, 0]
    assert got[:5] == [lib.UR_BRDF_LUT_MAX_WIDTH, lib.UR_BRDF_LUT_MAX_HEIGHT, lib.UR_BRDF_LUT_MIN_SAMPLES, lib.UR_BRDF_LUT_MAX_SAMPLES, lib.UR_BRDF_LUT_MAX_STREAM_OPS]


def test_refusals_that_need_no_device(urlib):
    """Every check comes before the context is looked at: a stand-in context is enough, the addresses are numbers and none is dereferenced.
    The host twin has the same refusals but for the context."""
    from unclerenderer_amd import lib
    stand_in = C.create_string_buffer(4096)
    w, h, s = 64, 8, 64
    ok = dict(ctx=C.addressof(stand_in), w=w, h=h, s=s, table=0x100000, table_bytes=16 * h * s, dst=0x300000, dst_bytes=4 * w * h)

    def refused(text, **kw):
        a = dict(ok, **kw)
        rc = urlib.ur_brdf_lut(a["ctx"], a["w"], a["h"], a["s"], a["table"], a["table_bytes"], a["dst"], a["dst_bytes"])
        said = urlib.ur_last_error().decode()
        assert rc == lib.UR_EINVAL and text in said, (text, kw, rc, said)
        if "ctx" not in kw:
            assert urlib.ur_host_brdf_lut(a["w"], a["h"], a["s"], a["table"], a["table_bytes"], a["dst"], a["dst_bytes"]) == lib.UR_EINVAL, kw

    refused("null context", ctx=None)
    refused("null table or destination", table=None)
    refused("null table or destination", dst=None)
    for bad in (0, 1025, 1 << 31):
        refused(f"a table of {bad} x {h}", w=bad)
    for bad in (0, 257, 1 << 31):
        refused(f"a table of {w} x {bad}", h=bad)
    for bad in (0, 8, 24, 48, 8192, 1 << 31):
        refused(f"sample count {bad}", s=bad)
    refused("table bytes", table_bytes=ok["table_bytes"] - 16)
    refused("table bytes", s=128)  # another table's size
    refused("destination bytes", dst_bytes=ok["dst_bytes"] - 4)
    refused("destination bytes", dst_bytes=ok["dst_bytes"] + 4)
    refused("destination bytes", w=w + 1)
    for off in (4, 8, 12):
        refused("table not 16-byte aligned", table=ok["table"] + off)
        refused("destination not 16-byte aligned", dst=ok["dst"] + off)
    refused("table and destination overlap", dst=ok["table"] + ok["table_bytes"] - 16)  # the destination begins in the table's last bytes
    refused("table and destination overlap", table=ok["dst"] + ok["dst_bytes"] - 16)    # the table begins in the destination's last bytes
    refused("table and destination overlap", table=ok["dst"])
    # a longer table is taken: only its first bytes are read (the addresses are not dereferenced by a refusal: nothing to run without a device)
    out = np.zeros(16 * h * s, np.uint8)
    at = C.c_void_p(out.ctypes.data)
    assert urlib.ur_host_brdf_lut_table(h, s, at, out.size) == 0 and out.any()
    assert urlib.ur_host_brdf_lut_table(h, s, at, out.size - 1) == lib.UR_EINVAL and urlib.ur_host_brdf_lut_table(h, s, None, out.size) == lib.UR_EINVAL
    for bad_h, bad_s in ((0, 64), (257, 64), (8, 0), (8, 48), (8, 8), (8, 8192)):
        assert urlib.ur_host_brdf_lut_table(bad_h, bad_s, at, out.size) == lib.UR_EINVAL and urlib.ur_brdf_lut_table_bytes(bad_h, bad_s) == 0


def test_python_functions_refuse(urlib):
    from unclerenderer_amd import environment, hostmath, hotpath

    class NoDevice(hotpath.HotPath):
        def __init__(self):
            self._L, self._ctx, self.device = urlib, None, 0
    hp = NoDevice()
    for w, h, s in ((0, 8, 64), (1025, 8, 64), (8, 0, 64), (8, 257, 64), (8, 8, 8), (8, 8, 48), (8, 8, 8192)):
        with pytest.raises(ValueError, match="no BRDF LUT"):
            environment.brdf_lut(hp, w, h, s)
        with pytest.raises(ValueError, match="no BRDF LUT table|ur_host_brdf_lut failed"):
            hostmath.brdf_lut(w, h, s)
    with pytest.raises(ValueError, match="no BRDF LUT table"):
        hostmath.brdf_lut_table(8, 100)
    with pytest.raises(ValueError, match="ur_host_brdf_lut failed"):
        hostmath.brdf_lut(8, 8, 64, table=hostmath.brdf_lut_table(4, 64))  # a short table
    lut = hostmath.brdf_lut(8, 4, 16)
    assert lut.shape == (4, 8, 2) and lut.dtype == np.uint16
