"""The kernels' metadata notes of the built library like tests/code_objects.py, but for every kernel whatever its linkage: a kernel with
C linkage stands in the notes under its plain name, which that reader (names that begin with _Z only) passes over. A kernel's record is
told from an argument's by its symbol: the notes name every kernel once more as `.symbol: <name>.kd`."""
import re
import subprocess
from pathlib import Path

from tests.code_objects import LLVM, code_objects

FIELDS = ("private_segment_fixed_size", "sgpr_spill_count", "vgpr_spill_count", "vgpr_count", "sgpr_count")


def kernel_metadata(co: Path) -> dict:
    """{kernel name, mangled or plain: {private_segment_fixed_size, sgpr_spill_count, vgpr_spill_count, vgpr_count, sgpr_count}}."""
    notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(co)], capture_output=True, text=True, check=True).stdout
    lines = [(m.group(1), m.group(2).strip().strip("'\"")) for m in (re.match(r"\s*-?\s*\.(\w+):\s*(.*)$", line) for line in notes.splitlines()) if m]
    symbols = {v[:-3] for k, v in lines if k == "symbol" and v.endswith(".kd")}
    kernels, cur = {}, None
    for k, v in lines:
        if k == "name" and v in symbols:
            cur = kernels.setdefault(v, {})
        elif cur is not None and k in FIELDS and v.isdigit():
            cur[k] = int(v)
    return kernels


def library_kernels(tmp_path: Path) -> dict:
    """kernel_metadata over every gfx950 code object of the built library."""
    from unclerenderer_amd import lib
    meta = {}
    for co in code_objects(lib.library_path(), tmp_path):
        meta.update(kernel_metadata(co))
    return meta
