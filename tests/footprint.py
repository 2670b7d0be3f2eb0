"""Footprint rules for the entry points of include/ur_hotpath.h: a kernel touches only the bytes its header names.

guarded() puts a payload in the middle of one larger allocation, between two guards of at least max(64 KiB, 16 image rows), so that
an overrun of a whole tile row or strip still lands inside the allocation. Two rules are built on it (run_rules):

  write rule  every buffer an entry point may write is guarded with a position-dependent fill (a hash of the byte offset and a
              seed: a stray store cannot hide by equalling a constant sentinel); after the call both guards are intact, and the
              parts of the payload the header says are left alone still hold what they held.
  read rule   every device input is guarded; the call runs with guards of 0xFF bytes ("ones": NaN as fp16 / fp32, the maximum as
              an integer) and with guards of zero bytes, and every output of the two runs is byte-equal to the other's and to the
              same call on plain tensors. A buffer that is read and written takes hash guards with a different seed per run.

The read rule sees a value from outside an input that reaches a result. It CANNOT see a stray load whose value is discarded
(a lane that loads past the end and masks the result off): that needs a fault or a tool, not a comparison. Values are not judged
here at all - the oracle and float64 tests do that; kernels are deterministic (the suite's own tests), so bytes are compared, NaN
payloads included, with no tolerance.

The module is device-agnostic (device "cpu" gives torch CPU tensors): tests/test_footprint_helper.py runs it without a GPU.

Entry points and the tests that hold them (tests/test_footprint_helper.py fails when an `int ur_*(` of the header that takes a
device pointer is missing here):

    ur_debug_stream_ceiling       tests/test_gpu_footprint_lighting.py::test_stream_ceiling_and_timeline_footprint
    ur_debug_timeline             tests/test_gpu_footprint_lighting.py::test_stream_ceiling_and_timeline_footprint
    ur_build_hzb                  tests/test_gpu_footprint_visibility.py::test_build_hzb_footprint
    ur_build_hzb_band             tests/test_gpu_footprint_visibility.py::test_build_hzb_band_and_tail_footprint
    ur_build_hzb_tail             tests/test_gpu_footprint_visibility.py::test_build_hzb_band_and_tail_footprint
    ur_cull_indirect_args         tests/test_gpu_footprint_visibility.py::test_cull_footprint
    ur_cull_indirect_args_ex      tests/test_gpu_footprint_visibility.py::test_cull_footprint
    ur_cull_indirect_args_draws   tests/test_gpu_footprint_visibility.py::test_cull_draws_and_views_read_rule
    ur_cull_indirect_args_views   tests/test_gpu_footprint_visibility.py::test_cull_draws_and_views_read_rule
    ur_stage_env_cube             tests/test_gpu_footprint_lighting.py::test_stage_env_cube_footprint
    ur_deferred_lighting          tests/test_gpu_footprint_lighting.py::test_lighting_shapes_footprint
    ur_sky_atmosphere             tests/test_gpu_footprint_lighting.py::test_lighting_shapes_footprint
    ur_deferred_lighting_sky      tests/test_gpu_footprint_lighting.py::test_lighting_shapes_footprint
    ur_tonemap                    tests/test_gpu_footprint_post.py::test_tonemap_footprint
    ur_temporal_aa                tests/test_gpu_footprint_post.py::test_temporal_aa_footprint
    ur_temporal_aa_tonemap        tests/test_gpu_footprint_post.py::test_temporal_aa_footprint
    ur_auto_exposure              tests/test_gpu_footprint_post.py::test_auto_exposure_footprint
    ur_cas                        tests/test_gpu_footprint_post.py::test_cas_footprint
    ur_tonemap_cas                tests/test_gpu_footprint_post.py::test_cas_footprint
    ur_pack_post_record           tests/test_gpu_footprint_post.py::test_pack_records_footprint
    ur_auto_exposure_records      tests/test_gpu_footprint_post.py::test_auto_exposure_footprint
    ur_tonemap_cas_halo           tests/test_gpu_footprint_post.py::test_cas_halo_footprint
    ur_cas_halo                   tests/test_gpu_footprint_post.py::test_cas_halo_footprint
    ur_pack_taa_record            tests/test_gpu_footprint_post.py::test_pack_records_footprint
    ur_temporal_aa_halo           tests/test_gpu_footprint_post.py::test_temporal_aa_halo_footprint
    ur_temporal_aa_tonemap_halo   tests/test_gpu_footprint_post.py::test_temporal_aa_halo_footprint
    ur_debug_print_reset          tests/test_gpu_footprint_frame.py::test_debug_print_footprint
    ur_debug_print_stats          tests/test_gpu_footprint_frame.py::test_debug_print_footprint
    ur_debug_print_text           tests/test_gpu_footprint_frame.py::test_debug_print_footprint
    ur_debug_print_draw           tests/test_gpu_footprint_frame.py::test_debug_print_footprint
    ur_allgather_rows             tests/test_gpu_footprint_frame.py::test_allgather_rows_footprint
    ur_allgather_rows_bytes       tests/test_gpu_footprint_frame.py::test_allgather_rows_footprint
    ur_allgather_rows_bytes_ex    tests/test_gpu_footprint_frame.py::test_allgather_rows_footprint
"""
from __future__ import annotations

import re
from dataclasses import dataclass

import numpy as np

MIN_GUARD = 64 * 1024
GUARD_ROWS = 16
GRAIN = 512  # what a fresh device allocation is aligned to: the payload keeps it under align=512, so the same kernel forms are chosen


def _torch():
    import torch
    return torch


def _as_tensor(a):
    """A CPU or device tensor of the payload; numpy unsigned types torch cannot hold are reinterpreted (bit patterns kept)."""
    torch = _torch()
    if isinstance(a, torch.Tensor):
        return a.contiguous()
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    elif a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a.copy())


def fill_bytes(n: int, fill, device, start: int = 0):
    """n guard bytes as a uint8 tensor: "ones", "zeros", or ("hash", seed) - byte i holds a hash of (start + i) mixed with seed."""
    torch = _torch()
    if fill == "ones":
        return torch.full((n,), 0xFF, dtype=torch.uint8, device=device)
    if fill == "zeros":
        return torch.zeros((n,), dtype=torch.uint8, device=device)
    kind, seed = fill
    assert kind == "hash"
    o = torch.arange(start, start + n, dtype=torch.int64, device=device)
    v = (o + 0x632BE5AB * (int(seed) + 1)) * 0x9E3779B1
    v = v ^ (v >> 29)
    v = v * 0x85EBCA6B
    v = v ^ (v >> 32)
    return (v & 0xFF).to(torch.uint8)


@dataclass
class Report:
    """What check() found: the guard bytes that changed, as offsets relative to the payload's first byte (negative: in front,
    >= nbytes: behind)."""
    nbytes: int
    row_bytes: int
    pixel_bytes: int
    offsets: np.ndarray  # int64, ascending

    @property
    def ok(self) -> bool:
        return self.offsets.size == 0

    @property
    def first(self):
        return int(self.offsets[0]) if self.offsets.size else None

    @property
    def last(self):
        return int(self.offsets[-1]) if self.offsets.size else None

    def where(self, off: int):
        """(row, column) of a byte offset, in image rows of the payload's width and in pixels; rows below 0 lie in front of the payload."""
        row = off // self.row_bytes
        return int(row), int((off - row * self.row_bytes) // self.pixel_bytes)

    def rows_touched(self):
        """The image rows (payload row numbering, continuing past its end and below zero) that hold a touched byte."""
        return sorted({int(o // self.row_bytes) for o in self.offsets.tolist()})

    def __str__(self):
        if self.ok:
            return "guards intact"
        f, l = self.first, self.last
        side = lambda o: "in front of" if o < 0 else "behind"  # noqa: E731
        return (f"{self.offsets.size} guard bytes touched: first at offset {f} ({side(f)} the payload of {self.nbytes} bytes; row, column "
                f"{self.where(f)}), last at offset {l} ({side(l)}; row, column {self.where(l)}); rows of {self.row_bytes} bytes")


class Footprint:
    """The allocation behind a guarded() view: alloc (uint8), the payload at [lo, lo + nbytes), guards on both sides."""

    def __init__(self, alloc, lo, nbytes, fill, row_bytes, pixel_bytes):
        self.alloc, self.lo, self.nbytes, self.fill = alloc, lo, nbytes, fill
        self.row_bytes, self.pixel_bytes = max(1, row_bytes), max(1, pixel_bytes)

    @property
    def hi(self):
        return self.lo + self.nbytes

    def check(self) -> Report:
        torch = _torch()
        total = self.alloc.numel()
        dev = self.alloc.device
        bad = []
        for a, b in ((0, self.lo), (self.hi, total)):
            diff = torch.nonzero(self.alloc[a:b] != fill_bytes(b - a, self.fill, dev, a)).reshape(-1)
            if diff.numel():
                bad.append(diff.cpu().numpy().astype(np.int64) + a - self.lo)
        offs = np.concatenate(bad) if bad else np.zeros(0, np.int64)
        return Report(self.nbytes, self.row_bytes, self.pixel_bytes, offs)


def guard_bytes(row_bytes: int) -> int:
    g = max(MIN_GUARD, GUARD_ROWS * row_bytes)
    return (g + GRAIN - 1) // GRAIN * GRAIN


def guarded(array_or_tensor, device, fill, align: int = 512, row_bytes: "int | None" = None):
    """The payload in the middle of one larger allocation on `device`; returns a contiguous view of exactly its shape and dtype.
    view.footprint is the Footprint (check(view) compares both guards). Guards are at least max(64 KiB, 16 rows) each, a multiple of
    512 (so of every `align`). align=512: the payload is 512-byte aligned like a fresh allocation; a smaller power of two: aligned to
    exactly that (address = align mod 512), for the forms a header documents for weaker alignments. row_bytes: the image row for the
    guard size and for reports; by default the bytes of payload[0] when it has two dimensions or more, else the element."""
    torch = _torch()
    src = _as_tensor(array_or_tensor)
    assert align > 0 and align & (align - 1) == 0 and align <= GRAIN and align % src.element_size() == 0, align
    nbytes = src.numel() * src.element_size()
    if row_bytes is None:
        row_bytes = (src[0].numel() if src.dim() >= 2 and src.shape[0] else 1) * src.element_size()
    pixel_bytes = (src[0, 0].numel() if src.dim() >= 3 and src.shape[0] and src.shape[1] else 1) * src.element_size()
    g = guard_bytes(row_bytes)
    total = g + GRAIN + nbytes + g + GRAIN
    alloc = torch.empty((total,), dtype=torch.uint8, device=device)
    want = align % GRAIN
    lo = g + (want - (alloc.data_ptr() + g)) % GRAIN
    alloc.copy_(fill_bytes(total, fill, alloc.device))
    payload = alloc[lo:lo + nbytes]
    payload.copy_(src.reshape(-1).view(torch.uint8).to(alloc.device))
    view = payload.view(src.dtype).view(src.shape)
    assert view.is_contiguous() and (alloc.data_ptr() + lo) % GRAIN == want
    assert nbytes == 0 or view.data_ptr() == alloc.data_ptr() + lo  # (an empty tensor's data_ptr() is null)
    view.footprint = Footprint(alloc, lo, nbytes, fill, row_bytes, pixel_bytes)
    return view


def check(view) -> Report:
    """Both guards of a guarded() view, byte for byte."""
    return view.footprint.check()


def host_bytes(t) -> np.ndarray:
    """A tensor's bytes on the host."""
    torch = _torch()
    return t.detach().contiguous().reshape(-1).view(torch.uint8).cpu().numpy()


def plain(a, device):
    """The payload on plain tensors: what every other test passes."""
    return _as_tensor(a).to(device)


def run_rules(call, inputs: dict, outputs: dict, device="cuda", aligns: "dict | None" = None, row_bytes: "dict | None" = None,
              untouched=None, what="", sync=None):
    """Both rules on one call.

    call(b): makes the entry-point call(s) on b[name] tensors (None stays None). inputs: name -> array the call only reads;
    outputs: name -> array with the buffer's initial content, for everything the call may write (read-and-written buffers too).
    aligns / row_bytes: per name, passed to guarded(). untouched(result) -> {name: boolean element mask}: the parts of outputs the
    header says are left alone, given the plain run's result (name -> array like outputs[name]); they must equal the initial content.
    Runs the call on plain tensors, with "ones" guards and with "zeros" guards; returns the plain run's outputs."""
    torch = _torch()
    aligns, row_bytes = aligns or {}, row_bytes or {}
    if sync is None:
        sync = torch.cuda.synchronize if str(device).startswith("cuda") else (lambda: None)
    init = {k: np.ascontiguousarray(v) for k, v in outputs.items() if v is not None}

    def collect(b):
        return {k: host_bytes(b[k]).view(init[k].dtype).reshape(init[k].shape) for k in init}

    b = {k: (plain(v, device) if v is not None else None) for k, v in {**inputs, **outputs}.items()}
    call(b)
    sync()
    base = collect(b)
    masks = untouched(base) if untouched is not None else {}
    for k, m in masks.items():
        assert np.array_equal(base[k][m], init[k][m]), f"{what}: {k}: a part the header leaves alone changed (plain tensors)"
    for run, poison in enumerate(("ones", "zeros")):
        b = {}
        for k, v in inputs.items():
            b[k] = guarded(v, device, poison, aligns.get(k, GRAIN), row_bytes.get(k)) if v is not None else None
        for k, v in outputs.items():
            b[k] = guarded(v, device, ("hash", 2 * hash_seed(k) + run), aligns.get(k, GRAIN), row_bytes.get(k)) if v is not None else None
        call(b)
        sync()
        for k in outputs:
            if b[k] is not None:
                r = check(b[k])
                assert r.ok, f"{what}: write rule, {k} ({poison} run): {r}"
        for k in inputs:  # an input is never written: its payload and its guards are as they were
            if b[k] is not None:
                r = check(b[k])
                assert r.ok, f"{what}: write rule, input {k} ({poison} run): {r}"
                assert np.array_equal(host_bytes(b[k]), host_bytes(_as_tensor(inputs[k]))), f"{what}: input {k} was written ({poison} run)"
        got = collect(b)
        for k in init:
            same = got[k].view(np.uint8) == base[k].view(np.uint8)
            if not same.all():
                at = np.flatnonzero(~same.reshape(-1))
                raise AssertionError(f"{what}: read rule, output {k} with {poison} guards differs from the plain run in {at.size} bytes, "
                                     f"first at byte {int(at[0])}, last at byte {int(at[-1])}")
        for k, m in masks.items():
            assert np.array_equal(got[k][m], init[k][m]), f"{what}: {k}: a part the header leaves alone changed ({poison} run)"
    return base


def hash_seed(name: str) -> int:
    """A small stable seed from a buffer's name (Python's hash() changes between processes)."""
    s = 0
    for ch in name:
        s = (s * 131 + ord(ch)) % 100003
    return s


def header_entry_points(header_text: str) -> list:
    """Names of the header's `int ur_*(` functions whose argument list has a pointer that may be device memory: every pointer
    argument other than the context, host structs of constants and the out-parameters of the host-only helpers."""
    out = []
    for m in re.finditer(r"^int (ur_\w+)\(([^;]*?)\);", header_text, re.M | re.S):
        name, args = m.group(1), re.sub(r"/\*.*?\*/", "", m.group(2), flags=re.S)
        if name in HOST_ONLY:
            continue
        device = False
        for a in args.split(","):
            a = a.strip()
            if "*" not in a or a.startswith(("ur_ctx*", "const ur_ctx*")):
                continue
            if re.match(r"const (ur_\w+_constants|ur_mip_desc|ur_lighting_tables|ur_draw_ranges|ur_cull_view|char)\*", a):
                continue
            if re.match(r"const uint32_t\* constants", a) or re.search(r"\*\s*(start_event|stop_event|comm)$", a):
                continue
            device = True
        if device:
            out.append(name)
    return out


# entry points whose pointers are all host memory (out-parameters, events)
HOST_ONLY = {"ur_debug_lighting_schedule", "ur_get_option", "ur_hzb_band_pieces", "ur_hzb_band_slices", "ur_time_next_lighting",
             "ur_time_next_cull"}


def table() -> dict:
    """entry point -> "file::test" from this module's docstring."""
    return dict(re.findall(r"^\s{4}(ur_\w+)\s+(tests/\S+::\w+)\s*$", __doc__, re.M))
