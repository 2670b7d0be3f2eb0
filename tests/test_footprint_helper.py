"""tests/footprint.py without a GPU: planted one-byte writes are found and located, alignment is as asked, the payload view aliases
the allocation, run_rules bites on a CPU stand-in for a kernel, and the table of entry points in the module's docstring is complete."""
import re
from pathlib import Path

import numpy as np
import pytest

from tests import footprint as F

ROOT = Path(__file__).resolve().parent.parent


def _image(h=5, w=7):
    return np.arange(h * w * 4, dtype=np.uint16).reshape(h, w, 4)


@pytest.mark.parametrize("fill", ["ones", "zeros", ("hash", 3)])
def test_planted_writes_are_found_and_located(fill):
    img = _image()
    v = F.guarded(img, "cpu", fill)
    fp = v.footprint
    assert F.check(v).ok and str(F.check(v)) == "guards intact"
    g_front, g_back = fp.lo, fp.alloc.numel() - fp.hi
    assert g_front >= F.MIN_GUARD and g_back >= F.MIN_GUARD
    row = 7 * 8
    for off, where in ((-1, (-1, 6)), (img.nbytes, (5, 0)), (-g_front, None), (img.nbytes + g_back - 1, None)):
        i = fp.lo + off
        old = int(fp.alloc[i])
        fp.alloc[i] = old ^ 0x40
        r = F.check(v)
        assert not r.ok and r.first == r.last == off and r.offsets.tolist() == [off], (off, str(r))
        assert r.where(off) == (off // row, (off % row) // 8)
        if where is not None:
            assert r.where(off) == where
        assert str(off) in str(r) and ("in front of" if off < 0 else "behind") in str(r)
        fp.alloc[i] = old
        assert F.check(v).ok
    # two writes: first and last, and the rows they lie in
    fp.alloc[fp.lo - 3] ^= 1
    fp.alloc[fp.hi + row + 2] ^= 1
    r = F.check(v)
    assert (r.first, r.last) == (-3, img.nbytes + row + 2) and r.rows_touched() == [-1, 6]


def test_hash_fill_depends_on_position_and_seed():
    a, b = F.fill_bytes(4096, ("hash", 1), "cpu"), F.fill_bytes(4096, ("hash", 2), "cpu")
    assert len(set(a.tolist())) > 200 and (a != b).float().mean() > 0.9
    assert F.fill_bytes(100, ("hash", 1), "cpu", 50).tolist() == a[50:150].tolist()
    assert set(F.fill_bytes(9, "ones", "cpu").tolist()) == {255} and set(F.fill_bytes(9, "zeros", "cpu").tolist()) == {0}


@pytest.mark.parametrize("align", [512, 256, 16, 8, 4])
def test_alignment_is_exactly_as_asked(align):
    v = F.guarded(_image(), "cpu", "zeros", align=align)
    assert v.data_ptr() % align == 0
    if align < 512:
        assert v.data_ptr() % (2 * align) != 0, "a weaker alignment is met exactly, not exceeded"
    assert v.footprint.lo % align == v.footprint.lo % align and v.footprint.lo >= F.MIN_GUARD


def test_guard_size_follows_the_image_width():
    assert F.guard_bytes(8) == F.MIN_GUARD
    assert F.guard_bytes(3840 * 8) == 16 * 3840 * 8 and F.guard_bytes(3840 * 8) % 512 == 0
    assert F.guard_bytes(6001 * 4) >= 16 * 6001 * 4 and F.guard_bytes(6001 * 4) % 512 == 0
    wide = np.zeros((2, 6001), np.float32)
    v = F.guarded(wide, "cpu", "ones")
    assert v.footprint.lo >= 16 * 6001 * 4 and v.footprint.alloc.numel() - v.footprint.hi >= 16 * 6001 * 4
    flat = F.guarded(np.zeros(10, np.float32), "cpu", "ones", row_bytes=6001 * 4)
    assert flat.footprint.lo >= 16 * 6001 * 4 and flat.footprint.row_bytes == 6001 * 4


def test_the_view_aliases_the_allocation():
    import torch
    img = _image()
    v = F.guarded(img, "cpu", ("hash", 0))
    fp = v.footprint
    assert v.shape == img.shape and v.dtype == torch.int16 and v.is_contiguous()
    assert v.data_ptr() == fp.alloc.data_ptr() + fp.lo
    assert np.array_equal(F.host_bytes(v), img.view(np.uint8).reshape(-1))
    v[2, 3, 1] = 0x1234
    at = fp.lo + ((2 * 7 + 3) * 4 + 1) * 2
    assert fp.alloc[at:at + 2].tolist() == [0x34, 0x12]
    assert F.check(v).ok, "a write inside the payload is not a guard hit"
    e = F.guarded(np.zeros((0, 4), np.float32), "cpu", "ones")
    assert e.numel() == 0 and F.check(e).ok
    t = F.guarded(torch.arange(6, dtype=torch.float32).reshape(2, 3), "cpu", "zeros")
    assert t.shape == (2, 3) and t.tolist() == [[0, 1, 2], [3, 4, 5]]


def test_run_rules_on_a_stand_in_kernel():
    """A CPU "kernel" that copies rows: clean, writing one element too many, and reading one element past its input."""
    src = np.arange(24, dtype=np.float32).reshape(4, 6)
    dst = np.full((4, 6), -1, np.float32)

    def through_alloc(t, start, n):
        fp = getattr(t, "footprint", None)
        if fp is None:  # plain tensors: stay inside
            return t.reshape(-1)[start:min(start + n, t.numel())]
        return fp.alloc[fp.lo + 4 * start: fp.lo + 4 * (start + n)].view(t.dtype)

    def clean(b):
        b["dst"][:3].copy_(b["src"][:3])

    out = F.run_rules(clean, {"src": src}, {"dst": dst}, device="cpu", untouched=lambda r: {"dst": np.arange(4)[:, None].repeat(6, 1) == 3})
    assert np.array_equal(out["dst"][:3], src[:3]) and (out["dst"][3] == -1).all()

    def overrun(b):
        clean(b)
        through_alloc(b["dst"], 24, 1).fill_(5.0)

    with pytest.raises(AssertionError, match=r"write rule, dst.*first at offset 96 \(behind.*row, column \(4, 0\)"):
        F.run_rules(overrun, {"src": src}, {"dst": dst}, device="cpu")

    def overread(b):
        b["dst"].reshape(-1)[:24].copy_(through_alloc(b["src"], 1, 24)[:24] if hasattr(b["src"], "footprint") else
                                        b["src"].reshape(-1).roll(-1))

    with pytest.raises(AssertionError, match="read rule, output dst"):
        F.run_rules(overread, {"src": src}, {"dst": dst}, device="cpu")

    def scribble(b):
        clean(b)
        b["dst"][3, 0] = 9

    with pytest.raises(AssertionError, match="leaves alone"):
        F.run_rules(scribble, {"src": src}, {"dst": dst}, device="cpu", untouched=lambda r: {"dst": np.arange(4)[:, None].repeat(6, 1) == 3})


def test_every_entry_point_with_a_device_pointer_has_a_footprint_test():
    header = (ROOT / "include" / "ur_hotpath.h").read_text()
    names = F.header_entry_points(header)
    assert len(names) >= 30 and "ur_tonemap" in names and "ur_debug_timeline" in names and "ur_get_option" not in names
    every = re.findall(r"^int (ur_\w+)\(", header, re.M)
    assert set(names) | F.HOST_ONLY | {"ur_reserve", "ur_defer_hzb_tail", "ur_flush", "ur_debug_set_hzb_timeout", "ur_time_cull_carried",
                                       "ur_set_option"} == set(every), "a header function is neither tabled nor known to be host-only"
    tab = F.table()
    missing = [n for n in names if n not in tab]
    assert not missing, f"no footprint test is named for {missing}: add one, and its row to the table in tests/footprint.py"
    for name, where in tab.items():
        path, test = where.split("::")
        text = (ROOT / path).read_text()
        m = re.search(rf"^def {test}\(.*?(?=^def |\Z)", text, re.M | re.S)
        assert m, f"{where} does not exist"
        assert re.search(rf"\b{name}\b", m.group(0)), f"{where} does not name {name} (its docstring lists the entry points it holds)"
