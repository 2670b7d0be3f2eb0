"""Draw ranges (ur_cull_indirect_args_draws, ur_frame_set_draw_ranges) without a GPU: the bound symbols, argument checks that need no
device, the ctypes struct against the C header's sizeof, the Python precondition check of the offsets, and scene.draw_offsets on the
shipped scenes."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
SCENES = ROOT / "tests" / "golden" / "assets" / "Scenes"
NEW = ("ur_cull_indirect_args_draws", "ur_frame_set_draw_ranges")


def test_new_symbols_are_declared_and_bound(urlib):
    from unclerenderer_amd import lib
    text = (ROOT / "include" / "ur_hotpath.h").read_text() + (ROOT / "include" / "ur_frame.h").read_text()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, text), name
        assert name in lib.SIGNATURES
        assert getattr(urlib, name).argtypes == lib.SIGNATURES[name][1]


def test_null_context_and_null_frame_are_rejected(urlib):
    from unclerenderer_amd import lib
    consts = (C.c_uint32 * lib.UR_CULL_CONSTANT_DWORDS)()
    dr = lib.DrawRanges(None, 1, None, None)
    assert urlib.ur_cull_indirect_args_draws(None, consts, None, None, None, None, None, None, None, 0, C.byref(dr)) == lib.UR_EINVAL
    assert urlib.ur_cull_indirect_args_draws(None, consts, None, None, None, None, None, None, None, 0, None) == lib.UR_EINVAL
    assert urlib.ur_frame_set_draw_ranges(None, None) == lib.UR_EINVAL
    assert urlib.ur_frame_set_draw_ranges(None, C.byref(dr)) == lib.UR_EINVAL
    assert "null" in urlib.ur_last_error().decode()


def _c_compiler():
    for c in (shutil.which("cc"), shutil.which("gcc"), "/opt/rocm/lib/llvm/bin/clang", shutil.which("clang")):
        if c and Path(c).exists():
            return c
    return None


def test_struct_matches_the_header(tmp_path):
    from unclerenderer_amd import lib
    text = (ROOT / "include" / "ur_hotpath.h").read_text()
    body = re.search(r"typedef struct ur_draw_ranges \{(.*?)\} ur_draw_ranges;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.findall(r"(\w+)\s*$", d.strip())[0] for d in body.split(";") if d.strip()]
    assert names == [n for n, _ in lib.DrawRanges._fields_]
    D = lib.DrawRanges
    assert C.sizeof(D) == 32 and (D.offsets.offset, D.range_count.offset, D.commands.offset, D.counts.offset) == (0, 8, 16, 24)
    cc = _c_compiler()
    assert cc is not None, "no C compiler to take sizeof(ur_draw_ranges)"
    src = tmp_path / "s.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ur_hotpath.h"\nint main(void) { printf("%zu %zu %zu %zu %zu\\n", '
                   "sizeof(ur_draw_ranges), offsetof(ur_draw_ranges, offsets), offsetof(ur_draw_ranges, range_count), "
                   "offsetof(ur_draw_ranges, commands), offsetof(ur_draw_ranges, counts)); return 0; }\n")
    exe = tmp_path / "s"
    subprocess.run([cc, "-std=c99", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(D), D.offsets.offset, D.range_count.offset, D.commands.offset, D.counts.offset]


def test_draw_offsets_from_keys():
    from unclerenderer_amd import scene
    assert scene.draw_offsets(np.arange(5)).tolist() == [0, 1, 2, 3, 4, 5]
    assert scene.draw_offsets([7, 7, 7]).tolist() == [0, 3]
    assert scene.draw_offsets([1, 1, 2, 1, 1, 3]).tolist() == [0, 2, 3, 5, 6]
    assert scene.draw_offsets([]).tolist() == [0, 0]
    assert scene.draw_offsets([4]).dtype == np.uint32


def test_offsets_precondition_is_checked_on_the_host():
    pytest.importorskip("torch")
    from unclerenderer_amd.hotpath import check_draw_offsets
    assert check_draw_offsets([0, 3, 3, 10], 10).tolist() == [0, 3, 3, 10]
    assert check_draw_offsets(np.array([0, 0], np.int64), 0).dtype == np.uint32
    for bad, n in (([0], 0), ([], 0), ([1, 10], 10), ([0, 5, 4, 10], 10), ([0, 9], 10), ([0, -1, 10], 10), ([0.0, 10.0], 10)):
        with pytest.raises(ValueError):
            check_draw_offsets(bad, n)


def test_sponza_is_one_command_per_reference_range(urlib):
    from unclerenderer_amd import scene
    sb = scene.load_scene_bounds(SCENES / "sponza.json")
    o = scene.draw_offsets(np.arange(sb.count))
    assert sb.count == 25 and o.size == 26 and (np.diff(o) == 1).all()


def test_pica_pica_pipeline_runs(urlib):
    from unclerenderer_amd import scene
    sb = scene.load_scene_bounds(SCENES / "pica_pica.json")
    keys = sb.pipeline_keys
    o = scene.draw_offsets(keys)
    runs = 1 + sum(1 for i in range(1, len(keys)) if keys[i] != keys[i - 1])  # counted independently: one run per key change
    assert sb.count == 170 and o.size == runs + 1 and o[0] == 0 and o[-1] == 170
    for a, b in zip(o[:-1], o[1:]):
        assert b > a and (keys[a:b] == keys[a]).all()
        assert b == len(keys) or keys[b] != keys[a]
