"""The gfx950 code objects inside the built library and their kernels' metadata notes, for the tests that hold a kernel to its resources
(no scratch, no spills, a register count). Reads the notes only, with the LLVM tools of the ROCm installation."""
import re
import struct
import subprocess
from pathlib import Path

LLVM = Path("/opt/rocm/lib/llvm/bin")


def code_objects(lib_path: Path, tmp_path: Path) -> list[Path]:
    """Every gfx950 code object of the library's offload bundles, written under tmp_path."""
    fat = tmp_path / "fat.bin"
    subprocess.run([str(LLVM / "llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", str(lib_path), str(tmp_path / "discard.so")], check=True)
    data, magic, out, pos = fat.read_bytes(), b"__CLANG_OFFLOAD_BUNDLE__", [], 0
    while (i := data.find(magic, pos)) >= 0:
        (n,) = struct.unpack_from("<Q", data, i + 24)
        o = i + 32
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", data, o)
            o += 24
            triple = data[o:o + tl].decode()
            o += tl
            if "gfx950" in triple and size:
                p = tmp_path / f"co_{len(out)}.elf"
                p.write_bytes(data[i + off:i + off + size])
                out.append(p)
        pos = i + len(magic)
    return out


def kernel_metadata(co: Path) -> dict:
    """{mangled kernel name: {private_segment_fixed_size, sgpr_spill_count, vgpr_spill_count, vgpr_count, sgpr_count}} of one code object."""
    notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(co)], capture_output=True, text=True, check=True).stdout
    kernels, cur = {}, None
    for line in notes.splitlines():
        m = re.match(r"\s*-?\s*\.(\w+):\s*(.*)$", line)
        if not m:
            continue
        k, v = m.group(1), m.group(2).strip().strip("'\"")
        if k == "name" and v.startswith("_Z") and not v.endswith(".kd"):
            cur = kernels.setdefault(v, {})
        elif cur is not None and k in ("private_segment_fixed_size", "sgpr_spill_count", "vgpr_spill_count", "vgpr_count", "sgpr_count") and v.isdigit():
            cur[k] = int(v)
    return kernels


def library_kernels(tmp_path: Path) -> dict:
    """kernel_metadata over every gfx950 code object of the built library."""
    from unclerenderer_amd import lib
    meta = {}
    for co in code_objects(lib.library_path(), tmp_path):
        meta.update(kernel_metadata(co))
    return meta
