"""Extra cull views (ur_cull_indirect_args_views, ur_frame_set_cull_views) without a GPU: the bound symbols, the ctypes struct against
the C header's sizeof, and every argument check that needs no device."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
NEW = ("ur_cull_indirect_args_views", "ur_frame_set_cull_views")


def test_new_symbols_are_declared_and_bound(urlib):
    from unclerenderer_amd import lib
    text = (ROOT / "include" / "ur_hotpath.h").read_text() + (ROOT / "include" / "ur_frame.h").read_text()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, text), name
        assert name in lib.SIGNATURES
        assert getattr(urlib, name).argtypes == lib.SIGNATURES[name][1]
    assert re.search(r"#define UR_MAX_CULL_VIEWS %d\b" % lib.UR_MAX_CULL_VIEWS, text)
    assert re.search(r"#define UR_FRAME_CULL_VIEWS 0x%xu\b" % lib.UR_FRAME_CULL_VIEWS, text)


def _c_compiler():
    for c in (shutil.which("cc"), shutil.which("gcc"), "/opt/rocm/lib/llvm/bin/clang", shutil.which("clang")):
        if c and Path(c).exists():
            return c
    return None


def test_struct_matches_the_header(tmp_path):
    from unclerenderer_amd import lib
    text = (ROOT / "include" / "ur_hotpath.h").read_text()
    body = re.search(r"typedef struct ur_cull_view \{(.*?)\} ur_cull_view;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.findall(r"(\w+)\s*(?:\[\d+\])?\s*$", d.strip())[0] for d in body.split(";") if d.strip()]
    V = lib.CullView
    assert names == [n for n, _ in V._fields_]
    cc = _c_compiler()
    assert cc is not None, "no C compiler to take sizeof(ur_cull_view)"
    src = tmp_path / "s.c"
    fields = ", ".join(f"offsetof(ur_cull_view, {n})" for n in names)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "ur_hotpath.h"\nint main(void) { printf("%zu'
                   + " %zu" * len(names) + '\\n", sizeof(ur_cull_view), ' + fields + "); return 0; }\n")
    exe = tmp_path / "s"
    subprocess.run([cc, "-std=c99", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(V)] + [getattr(V, n).offset for n in names]
    assert C.sizeof(V) == 128  # 24 floats, four pointers


def _consts(n):
    from unclerenderer_amd import lib
    c = (C.c_uint32 * lib.UR_CULL_CONSTANT_DWORDS)()
    c[40] = n
    return c


def _call(urlib, views, count, n=100, args=0x100000, draws=None):
    return urlib.ur_cull_indirect_args_views(None, _consts(n), None, None, None, C.c_void_p(args), None, None, None, 0,
                                             C.byref(draws) if draws is not None else None, views, count)


def _views(k):
    from unclerenderer_amd import lib
    return (lib.CullView * k)()


def _bad_cases():
    """(name, views, count, camera draws, expected words of the error). Fake device addresses: the checks come before the context."""
    from unclerenderer_amd import lib
    n, A = 100, 0x100000  # indirect_args at A, n * 64 = 6400 bytes
    cases = []
    v = _views(5)
    for x in v:
        x.mask = 0x900000
    cases.append(("too many", v, 5, None, "views"))
    v = _views(1)
    cases.append(("nothing", v, 1, None, "nothing"))
    v = _views(1); v[0].visible_idx = 0x900000
    cases.append(("list without count", v, 1, None, "together"))
    v = _views(1); v[0].visible_count = 0x900000
    cases.append(("count without list", v, 1, None, "together"))
    for member in ("offsets", "commands", "counts"):
        d = lib.DrawRanges(0x800000, 1, 0x900000, 0xA00000)
        setattr(d, member, None)
        v = _views(1); v[0].draws = C.pointer(d); v[0]._keep = d
        cases.append((f"null {member}", v, 1, None, "null"))
    d = lib.DrawRanges(0x800000, 0, 0x900000, 0xA00000)
    v = _views(1); v[0].draws = C.pointer(d); v[0]._keep = d
    cases.append(("no range", v, 1, None, "range"))
    d = lib.DrawRanges(0x800000, 1, A + 64 * (n - 1), 0xA00000)
    v = _views(1); v[0].draws = C.pointer(d); v[0]._keep = d
    cases.append(("overlaps indirect_args", v, 1, None, "overlap"))
    cam = lib.DrawRanges(0x800000, 1, 0x900000, 0xA00000)
    d = lib.DrawRanges(0x800000, 1, 0x900000 + 64, 0xA00000)
    v = _views(1); v[0].draws = C.pointer(d); v[0]._keep = d
    cases.append(("overlaps the camera's commands", v, 1, cam, "camera"))
    d0, d1 = lib.DrawRanges(0x800000, 1, 0x900000, 0xA00000), lib.DrawRanges(0x800000, 1, 0x900000 + 6384, 0xA00000)
    v = _views(2); v[0].draws = C.pointer(d0); v[1].draws = C.pointer(d1); v[0]._keep = (d0, d1)
    cases.append(("overlaps another view's", v, 2, None, "view 0"))
    d = lib.DrawRanges(0x800000, 1, 0x900008, 0xA00000)
    v = _views(1); v[0].draws = C.pointer(d); v[0]._keep = d
    cases.append(("commands misaligned", v, 1, None, "aligned"))
    v = _views(1); v[0].mask = 0x900002
    cases.append(("mask misaligned", v, 1, None, "aligned"))
    return cases


@pytest.mark.parametrize("case", range(len(_bad_cases())))
def test_invalid_views_are_rejected_before_anything_runs(urlib, case):
    from unclerenderer_amd import lib
    name, views, count, cam, words = _bad_cases()[case]
    assert _call(urlib, views, count, draws=cam) == lib.UR_EINVAL, name
    err = urlib.ur_last_error().decode()
    assert words in err and "ur_cull_indirect_args_views" in err, (name, err)


def test_frame_checks(urlib):
    from unclerenderer_amd import lib
    v = _views(1)
    v[0].mask = 0x900000
    assert urlib.ur_frame_set_cull_views(None, v, 1) == lib.UR_EINVAL
    assert "null frame" in urlib.ur_last_error().decode()
    assert urlib.ur_frame_set_cull_views(None, None, 0) == lib.UR_EINVAL


def test_a_valid_view_gets_as_far_as_the_context(urlib):
    """Nothing wrong with the views: the call fails only on the null context."""
    from unclerenderer_amd import lib
    v = _views(4)
    for i, x in enumerate(v):
        x.mask = 0x900000 + i * 0x1000
    assert _call(urlib, v, 4) == lib.UR_EINVAL
    assert "null ctx" in urlib.ur_last_error().decode()
    assert _call(urlib, None, 3) == lib.UR_EINVAL  # views == NULL: exactly ur_cull_indirect_args_draws
    assert "null ctx" in urlib.ur_last_error().decode()


def test_python_view_arguments_are_checked():
    pytest.importorskip("torch")
    from unclerenderer_amd import hotpath
    with pytest.raises(ValueError):
        hotpath.cull_view([0.0] * 23)
    with pytest.raises(ValueError):
        hotpath.cull_views_array([hotpath.cull_view([0.0] * 24)] * 5)
