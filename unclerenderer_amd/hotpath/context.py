"""The core of the context: creation and close, options, timers, Build HZB, the cull entry points, the lighting tables, Lighting and Sky."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .. import lib as _lib
from . import tensors
from .tensors import _ptr, nbytes


class HzbLayout:
    def __init__(self, src_w: int, src_h: int):
        self.src_w, self.src_h = src_w, src_h
        self.mips = (_lib.MipDesc * _lib.UR_MAX_HZB_MIPS)()
        n = C.c_uint32(0)
        self.total = int(_lib.load().ur_hzb_layout(src_w, src_h, self.mips, C.byref(n)))
        if self.total == 0:
            raise ValueError(f"bad HZB source size {src_w}x{src_h}")
        self.count = int(n.value)

    @property
    def width(self):
        return self.mips[0].width

    @property
    def height(self):
        return self.mips[0].height

    def as_list(self):
        return [(self.mips[i].offset, self.mips[i].width, self.mips[i].height) for i in range(self.count)]

    def mip_texels(self) -> int:
        return sum(self.mips[i].width * self.mips[i].height for i in range(self.count))

    def band_pieces(self, world: int, rank: int) -> tuple[int, int]:
        """(first piece row, piece rows) of the wide Build HZB launch that `rank` of `world` row bands builds (ur_hzb_band_pieces)."""
        a, b = C.c_uint32(0), C.c_uint32(0)
        _lib.check(_lib.load().ur_hzb_band_pieces(self.src_h, world, rank, C.byref(a), C.byref(b)), "ur_hzb_band_pieces")
        return int(a.value), int(b.value)

    def band_slices(self, piece_row0: int, piece_rows: int) -> list[tuple[int, int]]:
        """[(offset, count) in floats] of mips 0..4 for those piece rows (ur_hzb_band_slices): what a rank contributes to the exchange."""
        out = (_lib.HzbSlice * 5)()
        _lib.check(_lib.load().ur_hzb_band_slices(self.mips, self.count, piece_row0, piece_rows, out), "ur_hzb_band_slices")
        return [(int(s.offset), int(s.count)) for s in out]


class Context:
    """What every area's methods stand on: `_L` (the library), `_ctx` (the ur_ctx), `device` and `stream`."""

    def __init__(self, device: int | None = None, stream: "torch.cuda.Stream | None" = None):
        self._L = _lib.load()  # raises if the HIP extension is not built
        if not torch.cuda.is_available():
            raise RuntimeError("no HIP device visible: the hot path has no CPU fallback")
        self.device = torch.cuda.current_device() if device is None else device
        self.stream = stream if stream is not None else torch.cuda.current_stream(self.device)
        self._ctx = self._L.ur_create(self.device, C.c_void_p(self.stream.cuda_stream))
        if not self._ctx:
            raise RuntimeError("ur_create failed: " + self._L.ur_last_error().decode())

    def close(self):
        if getattr(self, "_ctx", None):
            self._L.ur_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def ctx(self):
        return self._ctx

    def set_option(self, option: int, value: int):
        """Launch-shape option of this context (lib.UR_OPT_*): results are the same bits under every value."""
        _lib.check(self._L.ur_set_option(self._ctx, option, value), "ur_set_option")

    def get_option(self, option: int) -> int:
        v = C.c_int(0)
        _lib.check(self._L.ur_get_option(self._ctx, option, C.byref(v)), "ur_get_option")
        return int(v.value)

    def lighting_schedule(self) -> dict:
        """Tile schedule of the last streaming Lighting launch on this context (ur_debug_lighting_schedule)."""
        out = (C.c_uint32 * 8)()
        _lib.check(self._L.ur_debug_lighting_schedule(self._ctx, out), "ur_debug_lighting_schedule")
        keys = ("groups", "tiles", "static_tiles", "pool_chunks", "chunk_shift", "lookahead", "waves_per_wg", "hzb_pieces")
        return dict(zip(keys, (int(v) for v in out)))

    def reserve(self, max_instances: int):
        _lib.check(self._L.ur_reserve(self._ctx, max_instances), "ur_reserve")

    def defer_hzb_tail(self, enable: "bool | int"):
        """1 / True: hold back the single-workgroup tail of build_hzb so that it rides along with the next streaming lighting
        launch; 2: hold back the whole chain (the lighting workgroups take the wide launch's pieces along too); 0: off."""
        _lib.check(self._L.ur_defer_hzb_tail(self._ctx, int(enable)), "ur_defer_hzb_tail")

    def debug_timeline(self, pairs: "torch.Tensor | None"):
        """pairs: (n, 2) int64 device tensor initialised to [-1, 0] rows (= {~0, 0} as uint64), or None to switch it off."""
        if pairs is None:
            _lib.check(self._L.ur_debug_timeline(self._ctx, None, 0), "ur_debug_timeline")
        else:
            assert pairs.dtype == torch.int64 and pairs.dim() == 2 and pairs.shape[1] == 2
            _lib.check(self._L.ur_debug_timeline(self._ctx, _ptr(pairs), pairs.shape[0]), "ur_debug_timeline")

    def flush(self):
        _lib.check(self._L.ur_flush(self._ctx), "ur_flush")

    def time_next_lighting(self, start: "torch.cuda.Event | None", stop: "torch.cuda.Event | None"):
        """The next Lighting launch carries this event pair on its kernel dispatch (ur_time_next_lighting): after a
        synchronise, start.elapsed_time(stop) is the dispatch's duration (launch included). The events must have been created
        with enable_timing=True and recorded once before (torch creates the HIP event lazily at its first record)."""
        if stop is None:
            _lib.check(self._L.ur_time_next_lighting(self._ctx, None, None), "ur_time_next_lighting")
        else:
            _lib.check(self._L.ur_time_next_lighting(self._ctx, C.c_void_p(start.cuda_event) if start is not None else None, C.c_void_p(stop.cuda_event)),
                       "ur_time_next_lighting")

    def stream_ceiling(self, ins, out, start: "torch.cuda.Event | None" = None, stop: "torch.cuda.Event | None" = None):
        """out = ins[0] + ins[1] + ins[2] + ins[3] on 16-byte elements (ur_debug_stream_ceiling): the plain streaming kernel whose
        rate bench.py --full prints as the practical ceiling. Events (recorded once before, like time_next_lighting's) ride on the dispatch."""
        assert len(ins) == 4 and all(nbytes(t) == nbytes(out) for t in ins)
        n16 = nbytes(out) // 16
        _lib.check(self._L.ur_debug_stream_ceiling(self._ctx, _ptr(ins[0]), _ptr(ins[1]), _ptr(ins[2]), _ptr(ins[3]), _ptr(out), n16,
                                                   C.c_void_p(start.cuda_event) if start is not None else None,
                                                   C.c_void_p(stop.cuda_event) if stop is not None else None), "ur_debug_stream_ceiling")

    # ---- BuildHZB ----
    def build_hzb(self, depth: torch.Tensor, hzb: torch.Tensor, layout: HzbLayout):
        assert depth.dtype == torch.float32 and hzb.dtype == torch.float32 and hzb.numel() >= layout.total
        assert depth.numel() == layout.src_w * layout.src_h
        _lib.check(self._L.ur_build_hzb(self._ctx, _ptr(depth), layout.src_w, layout.src_h, _ptr(hzb), layout.mips, layout.count), "ur_build_hzb")

    def build_hzb_band(self, depth: torch.Tensor, hzb: torch.Tensor, layout: HzbLayout, piece_row0: int, piece_rows: int):
        """Mips 0..4 for the 128x32 source pieces of rows [piece_row0, piece_row0 + piece_rows) only (ur_build_hzb_band)."""
        assert depth.dtype == torch.float32 and hzb.dtype == torch.float32 and hzb.numel() >= layout.total and depth.numel() == layout.src_w * layout.src_h
        _lib.check(self._L.ur_build_hzb_band(self._ctx, _ptr(depth), layout.src_w, layout.src_h, _ptr(hzb), layout.mips, layout.count, piece_row0, piece_rows),
                   "ur_build_hzb_band")

    def build_hzb_tail(self, hzb: torch.Tensor, layout: HzbLayout):
        """The single-workgroup rest of the chain (mips 5.. from mip 4), behind the ranks' exchange of the band slices (ur_build_hzb_tail)."""
        _lib.check(self._L.ur_build_hzb_tail(self._ctx, _ptr(hzb), layout.mips, layout.count), "ur_build_hzb_tail")

    # ---- CullIndirectArgs ----
    def cull_indirect_args(self, constants: np.ndarray, bounds: torch.Tensor, hzb, layout, indirect_args: torch.Tensor,
                           stats=None, visible_idx=None, visible_count=None, index_base: int = 0,
                           draw_offsets=None, draw_commands=None, draw_counts=None, views=None):
        """CullIndirectArgs (+ the optional visible list). With draw_offsets / draw_commands / draw_counts (all three or none) the same
        call also writes each range's visible commands to draw_commands slots draw_offsets[r], ... and its count to draw_counts[r]
        (ur_cull_indirect_args_draws). draw_offsets: a host array (checked here, then uploaded) or a device tensor from
        draw_offsets_to_device. views: up to UR_MAX_CULL_VIEWS extra frustum-only views (ur_cull_indirect_args_views), each a
        cull_view(...) or a dict of its arguments."""
        constants = np.ascontiguousarray(constants, np.uint32)
        assert constants.size == _lib.UR_CULL_CONSTANT_DWORDS
        cptr = constants.ctypes.data_as(C.POINTER(C.c_uint32))
        mips = layout.mips if layout is not None else None
        n = int(constants[40])
        with tensors.on_stream(self):  # (a view's host draw offsets are uploaded by cull_view)
            arr = cull_views_array([v if isinstance(v, _lib.CullView) else cull_view(command_count=n, **v) for v in views]) if views else None
        dr = None
        if draw_offsets is not None or draw_commands is not None or draw_counts is not None:
            if draw_offsets is None or draw_commands is None or draw_counts is None:
                raise ValueError("draw_offsets, draw_commands and draw_counts go together")
            if not isinstance(draw_offsets, torch.Tensor):
                draw_offsets = self.draw_offsets_to_device(draw_offsets, n)
            dr = draw_ranges(draw_offsets, draw_commands, draw_counts)
        where = "ur_cull_indirect_args_views" if views else "ur_cull_indirect_args_draws" if dr is not None else "ur_cull_indirect_args"
        # one entry point for every shape: views == NULL is exactly ur_cull_indirect_args_draws, draws == NULL exactly _ex
        _lib.check(self._L.ur_cull_indirect_args_views(self._ctx, cptr, _ptr(bounds), _ptr(hzb), mips, _ptr(indirect_args), _ptr(stats),
                                                       _ptr(visible_idx), _ptr(visible_count), index_base,
                                                       C.byref(dr) if dr is not None else None, arr, len(arr) if arr is not None else 0), where)

    def draw_offsets_to_device(self, offsets, command_count: int) -> torch.Tensor:
        """Check the precondition of ur_draw_ranges.offsets on the host array (offsets[0] == 0, non-decreasing, last == command_count,
        at least one range), then upload it (uint32)."""
        with tensors.on_stream(self):
            return tensors.to_device(check_draw_offsets(offsets, command_count), self.device)

    # ---- lighting tables ----
    def stage_env_cube(self, cube_dds_order: np.ndarray, base: int, mips: int) -> torch.Tensor:
        src = np.ascontiguousarray(cube_dds_order, np.uint16)
        n = int(self._L.ur_env_cube_texels(base, mips))
        if n == 0:
            raise ValueError("bad cube size")
        expect = 6 * sum(max(1, base >> m) ** 2 for m in range(mips))
        assert src.size == expect * 4, f"cube has {src.size // 4} texels, expected {expect}"
        with tensors.on_stream(self):
            dst = torch.empty((n, 4), dtype=torch.int16, device=f"cuda:{self.device}")
        _lib.check(self._L.ur_stage_env_cube(self._ctx, src.ctypes.data_as(C.c_void_p), base, mips, _ptr(dst)), "ur_stage_env_cube")
        return dst

    @staticmethod
    def make_tables(shadow, env_cube, env_base: int, env_mips: int, lut) -> _lib.LightingTables:
        t = _lib.LightingTables()
        t.shadow_map = shadow.data_ptr() if shadow is not None else None
        t.env_cube = env_cube.data_ptr()
        t.env_base_size, t.env_mip_count = env_base, env_mips
        t.env_cube_texels = nbytes(env_cube) // 8  # the staged buffer's size in half4 texels = the layout's tag
        t.brdf_lut_rg16 = lut.data_ptr()
        t.lut_height, t.lut_width = int(lut.shape[0]), int(lut.shape[1])
        t._keep = (shadow, env_cube, lut)  # keep the tensors alive
        return t

    # ---- DeferredLighting / SkyAtmosphere ----
    def deferred_lighting(self, scene, A, B, Cc, tables, hdr, w, h, row0=0, rows=None):
        rows = h - row0 if rows is None else rows
        _lib.check(self._L.ur_deferred_lighting(self._ctx, C.byref(scene), _ptr(A), _ptr(B), _ptr(Cc), C.byref(tables), _ptr(hdr), w, h, row0, rows),
                   "ur_deferred_lighting")

    def sky_atmosphere(self, sky, depth, hdr, w, h, row0=0, rows=None):
        rows = h - row0 if rows is None else rows
        _lib.check(self._L.ur_sky_atmosphere(self._ctx, C.byref(sky), _ptr(depth), _ptr(hdr), w, h, row0, rows), "ur_sky_atmosphere")

    def deferred_lighting_sky(self, scene, sky, A, B, Cc, depth, tables, hdr, w, h, row0=0, rows=None):
        rows = h - row0 if rows is None else rows
        _lib.check(self._L.ur_deferred_lighting_sky(self._ctx, C.byref(scene), C.byref(sky), _ptr(A), _ptr(B), _ptr(Cc), _ptr(depth), C.byref(tables),
                                                    _ptr(hdr), w, h, row0, rows), "ur_deferred_lighting_sky")


def check_draw_offsets(offsets, command_count: int) -> np.ndarray:
    """The precondition ur_cull_indirect_args_draws does not check, checked on the host: uint32[R + 1], R >= 1, offsets[0] == 0,
    non-decreasing, offsets[R] == command_count. Returns the array as contiguous uint32."""
    o = np.asarray(offsets)
    if o.ndim != 1 or o.size < 2:
        raise ValueError("draw offsets: need range_count + 1 >= 2 entries")
    if o.dtype.kind not in "iu" or (o.dtype.kind == "i" and (o < 0).any()) or (o > 0xFFFFFFFF).any():
        raise ValueError("draw offsets: must be unsigned 32-bit integers")
    o = np.ascontiguousarray(o, np.uint32)
    if o[0] != 0 or o[-1] != command_count or (np.diff(o.astype(np.int64)) < 0).any():
        raise ValueError(f"draw offsets: need offsets[0] == 0, non-decreasing, offsets[-1] == {command_count}")
    return o


def _host_draw_offsets(offsets, command_count: "int | None") -> torch.Tensor:
    """A host array of draw offsets, checked against command_count (by default its own last entry), on device 0: cull_view's and the frame's."""
    o = np.asarray(offsets)
    return tensors.to_device(check_draw_offsets(o, command_count if command_count is not None else (int(o[-1]) if o.size else -1)))


def draw_ranges(offsets: torch.Tensor, commands: torch.Tensor, counts: torch.Tensor) -> _lib.DrawRanges:
    """ur_draw_ranges over device tensors: offsets uint32[R + 1] (checked with check_draw_offsets), commands n * 64 bytes, counts uint32[R]."""
    assert offsets.numel() >= 2 and counts.numel() >= offsets.numel() - 1 and offsets.element_size() == 4 and counts.element_size() == 4
    dr = _lib.DrawRanges(offsets.data_ptr(), offsets.numel() - 1, commands.data_ptr(), counts.data_ptr())
    for t in (offsets, commands, counts):
        assert t.is_cuda and t.is_contiguous(), "device tensors must be contiguous CUDA/HIP tensors"
    dr._keep = (offsets, commands, counts)
    return dr


def cull_view(planes, mask=None, visible_idx=None, visible_count=None, draw_offsets=None, draw_commands=None, draw_counts=None,
              command_count: "int | None" = None) -> _lib.CullView:
    """ur_cull_view: 24 plane floats (hostmath.frustum_planes of the view's view-projection) and the device tensors the view writes:
    mask (uint32[ceil(n / 32)]), visible_idx + visible_count (both or neither), draw_offsets / draw_commands / draw_counts (all three or
    none; draw_offsets a host array checked with check_draw_offsets against command_count, or a device uint32 tensor). Keeps them alive."""
    p = np.ascontiguousarray(planes, np.float32).reshape(-1)
    if p.size != 24:
        raise ValueError("cull_view: planes must be 24 floats")
    if (visible_idx is None) != (visible_count is None):
        raise ValueError("cull_view: visible_idx and visible_count go together")
    v = _lib.CullView()
    v.planes[:] = p.tolist()
    keep = [t for t in (mask, visible_idx, visible_count) if t is not None]
    for t in keep:
        assert t.is_cuda and t.is_contiguous() and t.element_size() == 4, "view buffers must be contiguous 32-bit CUDA/HIP tensors"
    v.mask, v.visible_idx, v.visible_count = (t.data_ptr() if t is not None else None for t in (mask, visible_idx, visible_count))
    if draw_offsets is not None or draw_commands is not None or draw_counts is not None:
        if draw_offsets is None or draw_commands is None or draw_counts is None:
            raise ValueError("cull_view: draw_offsets, draw_commands and draw_counts go together")
        if not isinstance(draw_offsets, torch.Tensor):
            draw_offsets = _host_draw_offsets(draw_offsets, command_count)
        dr = draw_ranges(draw_offsets, draw_commands, draw_counts)
        v.draws = C.pointer(dr)
        keep.append(dr)
    v._keep = keep
    return v


def cull_views_array(views) -> "C.Array":
    """A ctypes ur_cull_view[] of cull_view(...) results, keeping them alive."""
    if len(views) > _lib.UR_MAX_CULL_VIEWS:
        raise ValueError(f"at most {_lib.UR_MAX_CULL_VIEWS} cull views")
    arr = (_lib.CullView * len(views))(*views)
    arr._keep = [getattr(v, "_keep", None) for v in views]
    return arr
