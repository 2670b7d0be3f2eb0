"""Python face of the C-ABI for device tensors (torch is used for device memory and streams only).

Method names follow the reference's passes: CullIndirectArgs (Renderer.cpp:394 DispatchGpuCulling), BuildHZB
(DeferredRenderer.cpp:998), DeferredLighting (:1219), SkyAtmosphere (:1263).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import lib as _lib


def _ptr(t):
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), "device tensors must be contiguous CUDA/HIP tensors"
    return C.c_void_p(t.data_ptr())


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


class HotPath:
    """One ur_ctx bound to a device and a stream."""

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
        assert len(ins) == 4 and all(t.numel() * t.element_size() == out.numel() * out.element_size() for t in ins)
        n16 = out.numel() * out.element_size() // 16
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
        return to_device(check_draw_offsets(offsets, command_count))

    # ---- lighting tables ----
    def stage_env_cube(self, cube_dds_order: np.ndarray, base: int, mips: int) -> torch.Tensor:
        src = np.ascontiguousarray(cube_dds_order, np.uint16)
        n = int(self._L.ur_env_cube_texels(base, mips))
        if n == 0:
            raise ValueError("bad cube size")
        expect = 6 * sum(max(1, base >> m) ** 2 for m in range(mips))
        assert src.size == expect * 4, f"cube has {src.size // 4} texels, expected {expect}"
        dst = torch.empty((n, 4), dtype=torch.int16, device=f"cuda:{self.device}")
        _lib.check(self._L.ur_stage_env_cube(self._ctx, src.ctypes.data_as(C.c_void_p), base, mips, _ptr(dst)), "ur_stage_env_cube")
        return dst

    @staticmethod
    def make_tables(shadow, env_cube, env_base: int, env_mips: int, lut) -> _lib.LightingTables:
        t = _lib.LightingTables()
        t.shadow_map = shadow.data_ptr() if shadow is not None else None
        t.env_cube = env_cube.data_ptr()
        t.env_base_size, t.env_mip_count = env_base, env_mips
        t.env_cube_texels = env_cube.numel() * env_cube.element_size() // 8  # the staged buffer's size in half4 texels = the layout's tag
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
            o = np.asarray(draw_offsets)
            draw_offsets = to_device(check_draw_offsets(o, command_count if command_count is not None else (int(o[-1]) if o.size else -1)))
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


class Frame:
    """The render-graph-driven frame (csrc/frame/HotPathRenderer.cpp): GPU Culling -> Build HZB -> Lighting -> Sky added to
    an FRenderGraph in the reference's order and executed on the context's stream."""

    def __init__(self, hp: HotPath, frames_in_flight: int = 3, rank: int = 0, world_size: int = 1):
        self._hp = hp
        self._L = hp._L
        self._f = self._L.ur_frame_create(hp.ctx, C.c_void_p(hp.stream.cuda_stream), frames_in_flight, rank, world_size)
        if not self._f:
            raise RuntimeError("ur_frame_create failed")
        self._keep = None

    def close(self):
        if getattr(self, "_f", None):
            self._L.ur_frame_destroy(self._f)
            self._f = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def resources(w, h, row0, rows, A, B, Cc, depth_band, lighting_band, depth_full, hzb, layout: HzbLayout, tables, bounds=None,
                  indirect_args=None, command_count=0, index_base=0, visible_idx=None, visible_count=None, cull_stats=None, tonemap_band=None):
        r = _lib.FrameResources()
        r.width, r.height, r.row0, r.rows = w, h, row0, rows
        dp = lambda t: t.data_ptr() if t is not None else None
        r.gbuffer_a, r.gbuffer_b, r.gbuffer_c = dp(A), dp(B), dp(Cc)
        r.depth_band, r.lighting_band, r.depth_full, r.hzb = dp(depth_band), dp(lighting_band), dp(depth_full), dp(hzb)
        if layout is not None:
            for i in range(layout.count):
                r.hzb_mips[i] = layout.mips[i]
            r.hzb_mip_count = layout.count
        r.tables = tables
        r.model_bounds, r.indirect_args = dp(bounds), dp(indirect_args)
        r.indirect_command_count, r.instance_index_base = command_count, index_base
        r.visible_indices, r.visible_count, r.cull_stats = dp(visible_idx), dp(visible_count), dp(cull_stats)
        r.tonemap_band = dp(tonemap_band)
        r._keep = (A, B, Cc, depth_band, lighting_band, depth_full, hzb, tables, bounds, indirect_args, visible_idx, visible_count, cull_stats, tonemap_band)
        return r

    def render(self, res, culling_constants: np.ndarray, scene, sky, flags: int = _lib.UR_FRAME_DEFAULT):
        cc = np.ascontiguousarray(culling_constants, np.uint32)
        _lib.check(self._L.ur_frame_render(self._f, C.byref(res), cc.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(scene), C.byref(sky), flags),
                   "ur_frame_render")

    def lighting_times_ms(self) -> np.ndarray:
        """Durations of the Lighting passes bracketed with UR_FRAME_TIME_LIGHTING since the last call (synchronise first)."""
        buf = np.zeros(1024, np.float32)
        n = self._L.ur_frame_lighting_times(self._f, _lib.fptr(buf), 1024)
        return buf[:n].copy()

    def lighting_times_and_record_cost_ms(self):
        """(bracket durations, cost of one event record behind each bracket) of the passes timed with UR_FRAME_TIME_LIGHTING."""
        buf, rec = np.zeros(1024, np.float32), np.zeros(1024, np.float32)
        n = self._L.ur_frame_lighting_times_ex(self._f, _lib.fptr(buf), _lib.fptr(rec), 1024)
        return buf[:n].copy(), rec[:n].copy()

    def join_async(self):
        self._L.ur_frame_join_async(self._f)

    @property
    def hzb_ready(self) -> bool:
        return bool(self._L.ur_frame_hzb_ready(self._f))

    def reset_hzb(self):
        self._L.ur_frame_reset_hzb(self._f)

    def set_post(self, luminance=(None, None), tonemap_scratch=None, delta_time=0.0, tonemap_exposure=0.9, tonemap_gamma=2.2, ae_key=0.3,
                 ae_min=0.1, ae_max=5.0, ae_speed_up=3.0, ae_speed_down=1.0, cas_sharpness=0.5):
        """ur_frame_set_post: the AutoExposure / CAS resources (device tensors, kept alive here) and parameters of the frames that follow."""
        dp = lambda t: t.data_ptr() if t is not None else None
        p = _lib.FramePost((C.c_void_p * 2)(dp(luminance[0]), dp(luminance[1])), dp(tonemap_scratch), delta_time, tonemap_exposure, tonemap_gamma,
                           ae_key, ae_min, ae_max, ae_speed_up, ae_speed_down, cas_sharpness)
        self._post_keep = (luminance, tonemap_scratch)
        _lib.check(self._L.ur_frame_set_post(self._f, C.byref(p)), "ur_frame_set_post")

    def reset_post(self):
        self._L.ur_frame_reset_post(self._f)

    def set_taa(self, history=None, history_weight=0.9):
        """ur_frame_set_taa: the TemporalAA history ring of the frames rendered with UR_FRAME_TAA - as many (height, width, 4) fp16
        device tensors as the frame has frames in flight (kept alive here), all invalid after the call. No history: clear."""
        if not history:
            self._taa_keep = None
            _lib.check(self._L.ur_frame_set_taa(self._f, None), "ur_frame_set_taa")
            return
        ptrs = (C.c_void_p * len(history))(*[t.data_ptr() if t is not None else None for t in history])
        t = _lib.FrameTaa(C.cast(ptrs, C.POINTER(C.c_void_p)), len(history), history_weight)
        _lib.check(self._L.ur_frame_set_taa(self._f, C.byref(t)), "ur_frame_set_taa")
        self._taa_keep = tuple(history)

    def taa_next(self) -> dict:
        """ur_frame_taa_next: {"read_slot", "write_slot", "use_history", "jitter"} of the next render with UR_FRAME_TAA; the caller
        jitters its projection with hostmath.apply_taa_jitter(proj, jitter, width, height) before it fills the frame's inputs."""
        i = _lib.FrameTaaInfo()
        _lib.check(self._L.ur_frame_taa_next(self._f, C.byref(i)), "ur_frame_taa_next")
        return {"read_slot": int(i.read_slot), "write_slot": int(i.write_slot), "use_history": bool(i.use_history),
                "jitter": np.array([i.jitter[0], i.jitter[1]], np.float32)}

    def reset_taa(self):
        """ur_frame_reset_taa: every history image invalid, sample index 0 (a resize)."""
        self._L.ur_frame_reset_taa(self._f)

    def set_draw_ranges(self, offsets=None, commands=None, counts=None, command_count: "int | None" = None):
        """ur_frame_set_draw_ranges: the "GPU Culling" pass of the frames that follow also writes each range's visible commands to
        `commands` slots offsets[r], ... and the range's count to counts[r] (device tensors, kept alive here). offsets: a host array
        (checked with check_draw_offsets against command_count, by default its own last entry, then uploaded) or a device uint32
        tensor. No arguments: clear."""
        if offsets is None and commands is None and counts is None:
            self._draws_keep = None
            _lib.check(self._L.ur_frame_set_draw_ranges(self._f, None), "ur_frame_set_draw_ranges")
            return
        if offsets is None or commands is None or counts is None:
            raise ValueError("offsets, commands and counts go together")
        if not isinstance(offsets, torch.Tensor):
            o = np.asarray(offsets)
            offsets = to_device(check_draw_offsets(o, command_count if command_count is not None else (int(o[-1]) if o.size else -1)))
        dr = draw_ranges(offsets, commands, counts)
        self._draws_keep = dr
        _lib.check(self._L.ur_frame_set_draw_ranges(self._f, C.byref(dr)), "ur_frame_set_draw_ranges")

    def set_cull_views(self, views=()):
        """ur_frame_set_cull_views: the "GPU Culling" pass of the frames rendered with UR_FRAME_CULL_VIEWS also culls these views
        (cull_view(...) results or dicts of its arguments; kept alive here). No views: clear."""
        views = [v if isinstance(v, _lib.CullView) else cull_view(**v) for v in views]
        arr = cull_views_array(views) if views else None
        self._views_keep = arr
        _lib.check(self._L.ur_frame_set_cull_views(self._f, arr, len(views)), "ur_frame_set_cull_views")

    def set_post_records(self, own_record, all_records):
        """ur_frame_set_post_records: where UR_FRAME_POST_EXCHANGE packs this rank's record (own_record) and where finish_post reads
        every rank's (all_records, rank order; own_record may be a view of its row). Device tensors, kept alive here."""
        self._records_keep = (own_record, all_records)
        _lib.check(self._L.ur_frame_set_post_records(self._f, C.c_void_p(own_record.data_ptr()), C.c_void_p(all_records.data_ptr())),
                   "ur_frame_set_post_records")

    def set_taa_records(self, own_record, all_records):
        """ur_frame_set_taa_records: where UR_FRAME_TAA_BAND packs this rank's TAA record (own_record, taa_record_bytes(w) bytes) and
        where finish_post reads every rank's (all_records, rank order; own_record may be a view of its row). Device tensors, kept alive
        here."""
        self._taa_records_keep = (own_record, all_records)
        _lib.check(self._L.ur_frame_set_taa_records(self._f, C.c_void_p(own_record.data_ptr()), C.c_void_p(all_records.data_ptr())),
                   "ur_frame_set_taa_records")

    def finish_post(self):
        """ur_frame_finish_post: the (TemporalAA /) AutoExposure / Tonemap / CAS passes of a frame rendered with UR_FRAME_POST_EXCHANGE, once
        the records are gathered."""
        _lib.check(self._L.ur_frame_finish_post(self._f), "ur_frame_finish_post")

    def report(self):
        """[(pass name, culled, transitions)] of the last executed graph."""
        n = self._L.ur_frame_report(self._f, None, 0)
        buf = C.create_string_buffer(n)
        self._L.ur_frame_report(self._f, buf, n)
        out = []
        for line in buf.value.decode().splitlines():
            name, culled, tr, *rest = line.split("|")
            out.append((name, culled == "1", int(tr)))
        return out

    def report_async(self):
        """[(pass name, ran on the async-compute stream, cross-stream waits)] of the last executed graph."""
        n = self._L.ur_frame_report(self._f, None, 0)
        buf = C.create_string_buffer(n)
        self._L.ur_frame_report(self._f, buf, n)
        return [(f[0], f[3] == "1", int(f[4])) for f in (l.split("|") for l in buf.value.decode().splitlines())]

    def timing_stats(self):
        n = self._L.ur_rg_timing_stats(None, 0)
        buf = C.create_string_buffer(n)
        self._L.ur_rg_timing_stats(buf, n)
        return [tuple(l.split("|")) for l in buf.value.decode().splitlines()]


def _tonemap(self, hdr, out_rgba8, w, rows, exposure=1.0, gamma=2.2, enable_tonemap=True, exposure_ev=None):
    """Tonemap pass (Tonemap.hlsl) over a band: RGBA16F -> R8G8B8A8_UNORM."""
    k = _tonemap_constants(enable_tonemap, exposure_ev, exposure, gamma)
    _lib.check(self._L.ur_tonemap(self._ctx, C.byref(k), _ptr(hdr), _ptr(exposure_ev), _ptr(out_rgba8), w, rows), "ur_tonemap")


HotPath.tonemap = _tonemap


def _temporal_aa(self, current_frame, history_band, output_band, history_weight, use_history, w, h, row0=0, rows=None):
    """TemporalAA resolve (TemporalAA.hlsl): current = full frame, history/output = band rows [row0,row0+rows)."""
    rows = h - row0 if rows is None else rows
    _lib.check(self._L.ur_temporal_aa(self._ctx, _ptr(current_frame), _ptr(history_band), _ptr(output_band), history_weight, int(use_history), w, h, row0, rows),
               "ur_temporal_aa")


HotPath.temporal_aa = _temporal_aa


def _temporal_aa_tonemap(self, current_frame, history_band, history_out_band, ldr_out_band, history_weight, use_history, w, h, row0=0, rows=None,
                         exposure=1.0, gamma=2.2, enable_tonemap=True, exposure_ev=None):
    """temporal_aa() followed by tonemap() of its output band, in one launch (the same bytes in history_out_band and ldr_out_band)."""
    rows = h - row0 if rows is None else rows
    k = _tonemap_constants(enable_tonemap, exposure_ev, exposure, gamma)
    _lib.check(self._L.ur_temporal_aa_tonemap(self._ctx, C.byref(k), _ptr(current_frame), _ptr(history_band), _ptr(history_out_band), _ptr(exposure_ev),
                                              _ptr(ldr_out_band), history_weight, int(use_history), w, h, row0, rows), "ur_temporal_aa_tonemap")


HotPath.temporal_aa_tonemap = _temporal_aa_tonemap


def _auto_exposure(self, hdr_full, out_ev, w, h, prev_ev=None, use_history=False, delta_time=0.0, speed_up=3.0, speed_down=1.0,
                   key=0.3, ev_min=0.1, ev_max=5.0):
    """AutoExposure (AutoExposure.hlsl) of the full RGBA16F frame: one float (the EV Tonemap applies) into out_ev.
    Defaults: RendererConfig.h:28-32."""
    k = _lib.AutoExposureConstants((C.c_float * 2)(w, h), delta_time, speed_up, speed_down, int(use_history), key, ev_min, ev_max)
    _lib.check(self._L.ur_auto_exposure(self._ctx, C.byref(k), _ptr(hdr_full), w, h, _ptr(prev_ev), _ptr(out_ev)), "ur_auto_exposure")


def _tonemap_constants(enable_tonemap, exposure_ev, exposure, gamma):
    return _lib.TonemapConstants(int(enable_tonemap), int(exposure_ev is not None), exposure, gamma)  # EnableAutoExposure: an EV texel is given


def _cas_constants(w, h, sharpness):
    return _lib.CasConstants((C.c_float * 2)(1.0 / w, 1.0 / h), sharpness, 0.0)  # TexelDelta as the pass sets it (DeferredRenderer.cpp:1533)


def _cas(self, ldr_full, out_band, w, h, row0=0, rows=None, sharpness=0.5):
    """CAS (Cas.hlsl) of rows [row0,row0+rows) of the full R8G8B8A8 image into a band-local output."""
    rows = h - row0 if rows is None else rows
    k = _cas_constants(w, h, sharpness)
    _lib.check(self._L.ur_cas(self._ctx, C.byref(k), _ptr(ldr_full), _ptr(out_band), w, h, row0, rows), "ur_cas")


def _tonemap_cas(self, hdr_full, out_band, w, h, row0=0, rows=None, exposure=1.0, gamma=2.2, enable_tonemap=True, exposure_ev=None,
                 sharpness=0.5):
    """Tonemap of the full frame then CAS of the band, in one launch (the same bytes as tonemap() followed by cas())."""
    rows = h - row0 if rows is None else rows
    tk = _tonemap_constants(enable_tonemap, exposure_ev, exposure, gamma)
    ck = _cas_constants(w, h, sharpness)
    _lib.check(self._L.ur_tonemap_cas(self._ctx, C.byref(tk), C.byref(ck), _ptr(hdr_full), _ptr(exposure_ev), _ptr(out_band), w, h, row0, rows),
               "ur_tonemap_cas")


HotPath.auto_exposure = _auto_exposure
HotPath.cas = _cas
HotPath.tonemap_cas = _tonemap_cas


# ---- the post exchange of row bands (include/ur_hotpath.h, ur_post_record_bytes) ----

def post_record_bytes(w: int) -> int:
    """Bytes of one rank's post record at width w: its first and last HDR rows and the 1024 AutoExposure tap texels, 8 B each."""
    return int(_lib.load().ur_post_record_bytes(w))


def _pack_post_record(self, hdr_band, record, w, h, row0, rows):
    """This band's post record (rows [row0,row0+rows) of the w x h frame) into `record` (post_record_bytes(w) bytes)."""
    _lib.check(self._L.ur_pack_post_record(self._ctx, _ptr(hdr_band), w, h, row0, rows, _ptr(record)), "ur_pack_post_record")


def _auto_exposure_records(self, records, n_ranks, out_ev, w, h, prev_ev=None, use_history=False, delta_time=0.0, speed_up=3.0, speed_down=1.0,
                           key=0.3, ev_min=0.1, ev_max=5.0):
    """auto_exposure of the whole frame from n_ranks gathered records (rank order): the same bits."""
    k = _lib.AutoExposureConstants((C.c_float * 2)(w, h), delta_time, speed_up, speed_down, int(use_history), key, ev_min, ev_max)
    _lib.check(self._L.ur_auto_exposure_records(self._ctx, C.byref(k), _ptr(records), n_ranks, w, h, _ptr(prev_ev), _ptr(out_ev)),
               "ur_auto_exposure_records")


def _tonemap_cas_halo(self, hdr_band, above, below, out_band, w, h, row0, rows, exposure=1.0, gamma=2.2, enable_tonemap=True, exposure_ev=None,
                      sharpness=0.5):
    """tonemap_cas of rows [row0,row0+rows) from the band and the HDR rows above / below it (None at the frame's edges)."""
    tk = _tonemap_constants(enable_tonemap, exposure_ev, exposure, gamma)
    ck = _cas_constants(w, h, sharpness)
    _lib.check(self._L.ur_tonemap_cas_halo(self._ctx, C.byref(tk), C.byref(ck), _ptr(hdr_band), _ptr(above), _ptr(below), _ptr(exposure_ev),
                                           _ptr(out_band), w, h, row0, rows), "ur_tonemap_cas_halo")


def _cas_halo(self, ldr_band, above, below, out_band, w, h, row0, rows, exposure=1.0, gamma=2.2, enable_tonemap=True, exposure_ev=None,
              sharpness=0.5):
    """cas of rows [row0,row0+rows) from tonemap()'s band output and the HDR rows above / below it, tonemapped with the same constants."""
    tk = _tonemap_constants(enable_tonemap, exposure_ev, exposure, gamma)
    ck = _cas_constants(w, h, sharpness)
    _lib.check(self._L.ur_cas_halo(self._ctx, C.byref(tk), C.byref(ck), _ptr(ldr_band), _ptr(above), _ptr(below), _ptr(exposure_ev),
                                   _ptr(out_band), w, h, row0, rows), "ur_cas_halo")


HotPath.post_record_bytes = staticmethod(post_record_bytes)
HotPath.pack_post_record = _pack_post_record
HotPath.auto_exposure_records = _auto_exposure_records
HotPath.tonemap_cas_halo = _tonemap_cas_halo
HotPath.cas_halo = _cas_halo


# ---- TemporalAA on row bands (include/ur_hotpath.h, ur_taa_record_bytes) ----

def taa_record_bytes(w: int) -> int:
    """Bytes of one rank's TAA record at width w: its second and second-last current rows and the first and last row of the history
    image it reads, 8 B a texel."""
    return int(_lib.load().ur_taa_record_bytes(w))


def _pack_taa_record(self, hdr_band, history_read_band, use_history, record, w, h, row0, rows):
    """This band's TAA record into `record` (taa_record_bytes(w) bytes); history_read_band may be None iff not use_history."""
    _lib.check(self._L.ur_pack_taa_record(self._ctx, _ptr(hdr_band), _ptr(history_read_band), int(use_history), w, h, row0, rows, _ptr(record)),
               "ur_pack_taa_record")


def _temporal_aa_halo(self, current_band, cur_above, cur_below, history_band, output_band, history_weight, use_history, w, h, row0, rows,
                      above2=None, hist_above=None, below2=None, hist_below=None, resolved_above=None, resolved_below=None):
    """temporal_aa of rows [row0,row0+rows) from the band and the current rows above / below it (None at the frame's edges); with
    resolved_above / resolved_below (and above2 / below2, hist_above / hist_below) the launch also resolves the rows around the band."""
    _lib.check(self._L.ur_temporal_aa_halo(self._ctx, _ptr(current_band), _ptr(cur_above), _ptr(cur_below), _ptr(history_band), _ptr(output_band),
                                           _ptr(above2), _ptr(hist_above), _ptr(below2), _ptr(hist_below), _ptr(resolved_above), _ptr(resolved_below),
                                           history_weight, int(use_history), w, h, row0, rows), "ur_temporal_aa_halo")


def _temporal_aa_tonemap_halo(self, current_band, cur_above, cur_below, history_band, history_out_band, ldr_out_band, history_weight, use_history,
                              w, h, row0, rows, above2=None, hist_above=None, below2=None, hist_below=None, resolved_above=None, resolved_below=None,
                              exposure=1.0, gamma=2.2, enable_tonemap=True, exposure_ev=None):
    """temporal_aa_halo() followed by tonemap() of its output band, in one launch."""
    k = _tonemap_constants(enable_tonemap, exposure_ev, exposure, gamma)
    _lib.check(self._L.ur_temporal_aa_tonemap_halo(self._ctx, C.byref(k), _ptr(current_band), _ptr(cur_above), _ptr(cur_below), _ptr(history_band),
                                                   _ptr(history_out_band), _ptr(exposure_ev), _ptr(ldr_out_band), _ptr(above2), _ptr(hist_above),
                                                   _ptr(below2), _ptr(hist_below), _ptr(resolved_above), _ptr(resolved_below), history_weight,
                                                   int(use_history), w, h, row0, rows), "ur_temporal_aa_tonemap_halo")


HotPath.taa_record_bytes = staticmethod(taa_record_bytes)
HotPath.pack_taa_record = _pack_taa_record
HotPath.temporal_aa_halo = _temporal_aa_halo
HotPath.temporal_aa_tonemap_halo = _temporal_aa_tonemap_halo


# ---- GpuDebugPrint (include/ur_hotpath.h, ur_debug_print_*) ----

def debug_print_buffer_bytes() -> int:
    """Bytes of the debug-print buffer: the entry count, then 4096 entries {x, y, code, color} of 16 bytes."""
    return int(_lib.load().ur_debug_print_buffer_bytes())


def debug_print_buffer(device=0) -> torch.Tensor:
    """A zeroed debug-print buffer as an int32 device tensor: [0] the count, [1 + 4 i : 5 + 4 i] entry i."""
    return torch.zeros(debug_print_buffer_bytes() // 4, dtype=torch.int32, device=f"cuda:{device}")


def _debug_print_reset(self, buffer, stats=None):
    """Zero the buffer's count and, when given, the cull's two counters (PrepareGpuDebugPrint)."""
    _lib.check(self._L.ur_debug_print_reset(self._ctx, _ptr(buffer), _ptr(stats)), "ur_debug_print_reset")


def _debug_print_stats(self, stats, buffer):
    """GpuDebugPrintStats.hlsl: "FRUSTUM n" / "OCCLUDE n" from stats[0] / stats[1] appended to the buffer."""
    _lib.check(self._L.ur_debug_print_stats(self._ctx, _ptr(stats), _ptr(buffer)), "ur_debug_print_stats")


def _debug_print_text(self, buffer, x, y, text, color=0xFFFFFFFF):
    """PrintString of `text` (str, encoded latin-1, or bytes) at (x, y): 8 pixels a character, stopping at a zero code."""
    raw = text.encode("latin-1") if isinstance(text, str) else bytes(text)
    _lib.check(self._L.ur_debug_print_text(self._ctx, _ptr(buffer), x, y, color, raw, len(raw)), "ur_debug_print_text")


def _debug_print_draw(self, buffer, glyphs, atlas, ldr, w, h, row0=0, rows=None, first_char=32, char_count=96):
    """GpuDebugPrint.hlsl's draw composited in place on rows [row0,row0+rows) of the w x h R8G8B8A8 image (ldr band-local).
    glyphs: (n, 10) float32 device tensor of ur_debug_glyph records indexed by code; atlas: (atlas_h, atlas_w) uint8 device tensor."""
    rows = h - row0 if rows is None else rows
    assert glyphs.dtype == torch.float32 and glyphs.dim() == 2 and glyphs.shape[1] == 10 and atlas.dtype == torch.uint8 and atlas.dim() == 2
    k = _lib.DebugPrintConstants((C.c_float * 2)(w, h), first_char, char_count)
    _lib.check(self._L.ur_debug_print_draw(self._ctx, C.byref(k), _ptr(glyphs), glyphs.shape[0], _ptr(atlas), atlas.shape[1], atlas.shape[0],
                                           _ptr(buffer), _ptr(ldr), w, h, row0, rows), "ur_debug_print_draw")


HotPath.debug_print_buffer_bytes = staticmethod(debug_print_buffer_bytes)
HotPath.debug_print_reset = _debug_print_reset
HotPath.debug_print_stats = _debug_print_stats
HotPath.debug_print_text = _debug_print_text
HotPath.debug_print_draw = _debug_print_draw


def _frame_set_debug_print(self, buffer=None, glyphs=None, atlas=None, first_char=32, char_count=96):
    """ur_frame_set_debug_print: the text buffer and font (device tensors as in HotPath.debug_print_draw, kept alive here) of the frames
    rendered with UR_FRAME_DEBUG_PRINT. No arguments: clear."""
    if buffer is None and glyphs is None and atlas is None:
        self._debug_print_keep = None
        _lib.check(self._L.ur_frame_set_debug_print(self._f, None), "ur_frame_set_debug_print")
        return
    dp = _lib.FrameDebugPrint(buffer.data_ptr() if buffer is not None else None, glyphs.data_ptr() if glyphs is not None else None,
                              glyphs.shape[0] if glyphs is not None else 0, atlas.data_ptr() if atlas is not None else None,
                              atlas.shape[1] if atlas is not None else 0, atlas.shape[0] if atlas is not None else 0, first_char, char_count)
    _lib.check(self._L.ur_frame_set_debug_print(self._f, C.byref(dp)), "ur_frame_set_debug_print")
    self._debug_print_keep = (buffer, glyphs, atlas)


Frame.set_debug_print = _frame_set_debug_print


# ---- ShadowMap (include/ur_raster.h) ----

def pack_draw_commands(draws) -> np.ndarray:
    """FIndirectDrawCommand slots (RendererUtils.h:102-111) as uint32[n, 16] from dicts of device tensors and numbers:
    vertices (any contiguous tensor; the view is its whole storage unless vertex_bytes says less), stride (bytes of a vertex, 64 in the
    reference), indices (int32 / uint32 tensor), constants (tensor whose first 64 bytes are World; constants_offset bytes into it),
    index_count (default: every index behind start_index), instance_count (1), start_index (0), base_vertex (0), index_format (42 =
    R32_UINT). Upload the result with to_device; the tensors must outlive the commands that point at them."""
    out = np.zeros((len(draws), 16), np.uint32)
    for row, d in zip(out, draws):
        v, i, c = d["vertices"], d["indices"], d["constants"]
        for t in (v, i, c):
            assert t.is_cuda and t.is_contiguous(), "device tensors must be contiguous CUDA/HIP tensors"
        va, ia, ca = v.data_ptr(), i.data_ptr(), c.data_ptr() + int(d.get("constants_offset", 0))
        index_slots = i.numel() * i.element_size() // 4
        start = int(d.get("start_index", 0))
        row[0], row[1] = va & 0xFFFFFFFF, va >> 32
        row[2] = int(d.get("vertex_bytes", v.numel() * v.element_size()))
        row[3] = int(d.get("stride", 64))
        row[4], row[5] = ia & 0xFFFFFFFF, ia >> 32
        row[6] = int(d.get("index_bytes", index_slots * 4))
        row[7] = int(d.get("index_format", _lib.UR_RASTER_INDEX_FORMAT_R32_UINT))
        row[8], row[9] = ca & 0xFFFFFFFF, ca >> 32
        row[10] = int(d.get("index_count", max(index_slots - start, 0)))
        row[11] = int(d.get("instance_count", 1))
        row[12] = start
        row[13] = np.int64(d.get("base_vertex", 0)).astype(np.int32).view(np.uint32)
    return out


def raster_draws(commands, command_count=None, visible=None, ranges=None, index_base=0) -> _lib.RasterDraws:
    """ur_raster_draws over device tensors. commands: n * 64 bytes (None with ranges). visible: (visible_idx, visible_count) device
    tensors. ranges: a draw_ranges(...) result, or (offsets, commands, counts) device tensors. Keeps them alive. The slots, and so the
    default command_count, live where the native ur::raster_commands says: in the ranges' commands if ranges are given, else in `commands`."""
    d = _lib.RasterDraws()
    keep = [commands]
    if commands is not None:
        assert commands.is_cuda and commands.is_contiguous()
        d.commands = commands.data_ptr()
    if ranges is not None and not isinstance(ranges, _lib.DrawRanges):
        ranges = draw_ranges(*ranges)
    if command_count is None:
        src = ranges._keep[1] if ranges is not None else commands
        command_count = src.numel() * src.element_size() // _lib.UR_INDIRECT_COMMAND_STRIDE if src is not None else 0
    d.command_count = int(command_count)
    if visible is not None:
        idx, cnt = visible
        d.visible_idx = idx.data_ptr() if idx is not None else None
        d.visible_count = cnt.data_ptr() if cnt is not None else None
        keep += [idx, cnt]
    d.index_base = int(index_base)
    if ranges is not None:
        d.ranges = C.pointer(ranges)
        keep.append(ranges)
    d._keep = keep
    return d


def _matrix16(m) -> np.ndarray:
    """16 contiguous floats of a 4 x 4 matrix (row-major, row-vector convention)."""
    a = np.ascontiguousarray(m, np.float32).reshape(-1)
    assert a.size == 16
    return a


def _shadow_map(self, lvp, commands, shadow_map, *, visible=None, ranges=None, index_base=0, stats=None, command_count=None, size=None):
    """ur_shadow_map: clear shadow_map ((h, w) float32 device tensor, or flat with size=(w, h)) to 1.0 and rasterise the selected draws
    of `commands` (pack_draw_commands, uploaded) under the orthographic light matrix lvp (16 floats, row-major, row-vector
    convention). visible=(visible_idx, visible_count) or ranges=(offsets, commands, counts) select; stats: uint32[4] device tensor,
    added to."""
    w, h = size if size is not None else (int(shadow_map.shape[1]), int(shadow_map.shape[0]))
    assert shadow_map.dtype == torch.float32 and shadow_map.numel() >= w * h
    m = _matrix16(lvp)
    d = raster_draws(commands, command_count, visible, ranges, index_base)
    _lib.check(self._L.ur_shadow_map(self._ctx, _lib.fptr(m), C.byref(d), _ptr(shadow_map), w, h, _ptr(stats)), "ur_shadow_map")


def _raster_reserve(self, max_large_work_items: int):
    """ur_raster_reserve: room for that many (triangle, 64 x 64 tile) entries of the large-triangle queue; 0 frees it."""
    _lib.check(self._L.ur_raster_reserve(self._ctx, int(max_large_work_items)), "ur_raster_reserve")


def _depth_prepass(self, view, projection, commands, depth, *, visible=None, ranges=None, index_base=0, stats=None, command_count=None, size=None,
                   flags=0):
    """ur_depth_prepass: clear depth ((h, w) float32 device tensor, or flat with size=(w, h)) to 0.0 and rasterise the selected draws of
    `commands` under the camera's view and projection (16 floats each, row-major, row-vector convention; reverse-Z), keeping the
    per-texel maximum. The selections are HotPath.shadow_map's; stats: uint32[6] device tensor, added to; flags: UR_DEPTH_QUANTIZE_D24."""
    w, h = size if size is not None else (int(depth.shape[1]), int(depth.shape[0]))
    assert depth.dtype == torch.float32 and depth.numel() >= w * h
    v, p = _matrix16(view), _matrix16(projection)
    d = raster_draws(commands, command_count, visible, ranges, index_base)
    _lib.check(self._L.ur_depth_prepass(self._ctx, _lib.fptr(v), _lib.fptr(p), C.byref(d), _ptr(depth), w, h, int(flags), _ptr(stats)), "ur_depth_prepass")


def gbuffer_targets(gbuf_a, gbuf_b, gbuf_c, hdr, keys, object_id=None) -> _lib.GBufferTargets:
    """ur_gbuffer_targets over device tensors of the band (rows x w): gbuf_a, gbuf_b, hdr float16 (..., 4), gbuf_c, keys and the optional
    object_id int32. Keeps them alive."""
    for t in (gbuf_a, gbuf_b, hdr):
        assert t.dtype == torch.float16 and t.is_contiguous()
    for t in (gbuf_c, keys) + ((object_id,) if object_id is not None else ()):
        assert t.dtype == torch.int32 and t.is_contiguous()
    tg = _lib.GBufferTargets(gbuf_a.data_ptr(), gbuf_b.data_ptr(), gbuf_c.data_ptr(), hdr.data_ptr(),
                             object_id.data_ptr() if object_id is not None else None, keys.data_ptr())
    tg._keep = (gbuf_a, gbuf_b, gbuf_c, hdr, keys, object_id)
    return tg


class Texture:
    """A texture on the device: the packed levels (`buffer`, kept alive here) and their ur_texture2d descriptor (`desc`)."""

    def __init__(self, buffer, desc):
        self.buffer, self.desc = buffer, desc


def pack_texture(levels, srgb: bool) -> Texture:
    """A list of (h, w, 4) uint8 arrays, level 0 first, level k max(1, w >> k) x max(1, h >> k), becomes one device buffer of tightly
    packed texels and its descriptor (UR_TEXTURE_R8G8B8A8_UNORM_SRGB when srgb, else UR_TEXTURE_R8G8B8A8_UNORM)."""
    levels = [np.ascontiguousarray(a, np.uint8) for a in levels]
    h0, w0 = levels[0].shape[:2]
    assert 1 <= len(levels) <= 255 and 1 <= w0 <= 65535 and 1 <= h0 <= 65535
    for k, a in enumerate(levels):
        assert a.shape == (max(1, h0 >> k), max(1, w0 >> k), 4), f"level {k} is {a.shape}"
    buffer = to_device(np.concatenate([a.reshape(-1) for a in levels]).view(np.uint32))
    desc = _lib.Texture2D(buffer.data_ptr(), w0, h0, len(levels), _lib.UR_TEXTURE_R8G8B8A8_UNORM_SRGB if srgb else _lib.UR_TEXTURE_R8G8B8A8_UNORM, 0)
    return Texture(buffer, desc)


def pack_texture_bc(payload, width: int, height: int, mips: int, format: int) -> Texture:
    """A chain of BC1 / BC3 / BC5 blocks (bytes or a uint8 array: a DDS file's payload as it lies, level 0 first, no padding) becomes one device
    buffer and its descriptor. `format` is one of lib.UR_TEXTURE_BC*; the length must be what hostmath.bc_chain_bytes gives for the chain."""
    from . import hostmath
    data = np.frombuffer(bytes(payload), np.uint8) if isinstance(payload, (bytes, bytearray, memoryview)) else np.ascontiguousarray(payload, np.uint8).reshape(-1)
    need = hostmath.bc_chain_bytes(format, width, height, mips)
    if need == 0:
        raise ValueError(f"no BC chain: format {format}, {width} x {height}, {mips} mips (UR_TEXTURE_BC*, sizes 1..65535, mips 1..255)")
    if data.size != need:
        raise ValueError(f"a {width} x {height} chain of {mips} mips in format {format} is {need} bytes, the payload has {data.size}")
    buffer = to_device(data.copy())  # (torch allocations are aligned far beyond a block's 16 bytes)
    assert buffer.data_ptr() % 16 == 0
    return Texture(buffer, _lib.Texture2D(buffer.data_ptr(), width, height, mips, int(format), 0))


class Materials:
    """A ur_material table on the device: `table` (int32 tensor, 20 dwords per record), `count`, and the textures it points to."""

    def __init__(self, table, count, keep):
        self.table, self.count, self._keep = table, count, keep


def pack_materials(materials) -> Materials:
    """[{"key": pipeline key, "base_color" / "metallic_roughness" / "normal" / "emissive": a Texture, a lib.Texture2D or None}, ...], one
    per command slot, becomes the device table HotPath.gbuffer_pass(materials=) and Frame.set_gbuffer_materials take. A key is 0-31: bit 4
    (UR_MATERIAL_ALPHA_MASK) is looked at for the slots of gbuffer_pass(mask_draws=) only."""
    rec = (_lib.Material * max(len(materials), 1))()
    keep = []
    for r, m in zip(rec, materials):
        r.pipeline_key = int(m.get("key", 0))
        assert 0 <= r.pipeline_key <= 31, f"pipeline key {r.pipeline_key} (0-31)"
        for name in ("base_color", "metallic_roughness", "normal", "emissive"):
            t = m.get(name)
            if t is None:
                continue
            keep.append(t)
            setattr(r, name, t.desc if isinstance(t, Texture) else t)
    host = np.frombuffer(bytes(rec), np.uint32).copy()
    return Materials(to_device(host), len(materials), keep)


def _gbuffer_pass(self, view, projection, commands, depth, targets, w, h, row0=0, rows=None, *, visible=None, ranges=None, index_base=0, stats=None,
                  command_count=None, flags=0, key_triangle_bits=0, parts=None, materials=None, mask_draws=None, keys64=None, mask_stats=None, won=None):
    """ur_gbuffer_pass: rasterise the selected draws of `commands` (64-byte vertices, whole ur_scene_constants behind the constant address)
    into visibility keys against `depth` (the w x h result of depth_prepass, read only) and resolve the rows [row0, row0 + rows) into
    `targets` (gbuffer_targets(...)). The selections are HotPath.shadow_map's; stats: uint32[6] device tensor, added to; flags:
    UR_DEPTH_QUANTIZE_D24; key_triangle_bits: the key's triangle bits, 0 = 32 - bit_length(command_count). parts: None, or for a timing tool
    UR_GBUFFER_PART_RASTER and / or UR_GBUFFER_PART_RESOLVE through ur_gbuffer_pass_parts (the resolve part alone trusts targets.keys).
    materials: a pack_materials(...) table, one record per command slot: the textured resolve of ur_gbuffer_pass_materials.
    mask_draws: a raster_draws(...) selection of the alpha-masked models over the same commands: ur_gbuffer_pass_masked, which applies the
    alpha test to the slots whose key has UR_MATERIAL_ALPHA_MASK, writes `depth` where a masked fragment wins and needs keys64, an int64
    (rows, w) device tensor of scratch; mask_stats: uint32[6] and won: uint32[1] device tensors, added to."""
    rows = h - row0 if rows is None else rows
    assert depth.dtype == torch.float32 and depth.numel() >= w * h
    v, p = _matrix16(view), _matrix16(projection)
    d = raster_draws(commands, command_count, visible, ranges, index_base)
    args = (self._ctx, _lib.fptr(v), _lib.fptr(p), C.byref(d), _ptr(depth), C.byref(targets), w, h, int(row0), int(rows), int(flags), int(key_triangle_bits),
            _ptr(stats))
    if mask_draws is not None:
        assert keys64 is not None and keys64.dtype == torch.int64 and keys64.is_contiguous() and keys64.numel() >= w * rows
        mask = _lib.GBufferMask(C.pointer(mask_draws), keys64.data_ptr(), _ptr(mask_stats), _ptr(won))
        table, count = (None, 0) if materials is None else ((materials.table, materials.count) if isinstance(materials, Materials) else materials)
        if parts is None:
            _lib.check(self._L.ur_gbuffer_pass_masked(*args, _ptr(table), int(count), C.byref(mask)), "ur_gbuffer_pass_masked")
        else:
            _lib.check(self._L.ur_gbuffer_pass_masked_parts(*args, int(parts), _ptr(table), int(count), C.byref(mask)), "ur_gbuffer_pass_masked_parts")
    elif materials is not None:
        table, count = (materials.table, materials.count) if isinstance(materials, Materials) else materials
        if parts is None:
            _lib.check(self._L.ur_gbuffer_pass_materials(*args, _ptr(table), int(count)), "ur_gbuffer_pass_materials")
        else:
            _lib.check(self._L.ur_gbuffer_pass_materials_parts(*args, int(parts), _ptr(table), int(count)), "ur_gbuffer_pass_materials_parts")
    elif parts is None:
        _lib.check(self._L.ur_gbuffer_pass(*args), "ur_gbuffer_pass")
    else:
        _lib.check(self._L.ur_gbuffer_pass_parts(*args, int(parts)), "ur_gbuffer_pass_parts")


def forward_targets(hdr, keys) -> _lib.ForwardTargets:
    """ur_forward_targets over device tensors of the band (rows x w): hdr float16 (..., 4), keys int32. Keeps them alive."""
    assert hdr.dtype == torch.float16 and hdr.is_contiguous() and keys.dtype == torch.int32 and keys.is_contiguous()
    tg = _lib.ForwardTargets(hdr.data_ptr(), keys.data_ptr())
    tg._keep = (hdr, keys)
    return tg


def _forward_pass(self, view, projection, commands, depth, targets, w, h, row0=0, rows=None, *, scene, tables, visible=None, ranges=None, index_base=0,
                  stats=None, command_count=None, flags=0, key_triangle_bits=0, parts=None, materials=None, mask_draws=None, keys64=None, mask_stats=None,
                  won=None):
    """ur_forward_pass: HotPath.gbuffer_pass' raster (with mask_draws, the masked raster and the merge that raises `depth`), then the forward
    resolve of the rows [row0, row0 + rows) into targets.hdr (forward_targets(...)) where a key won; the other texels keep what sky_atmosphere
    drew before. scene: a lib.SceneConstants whose per-frame fields are read (light, camera, LightViewProjection, the shadow fields,
    EnvMapMipCount; the per-draw ones come from each command's own block); tables: make_tables(...). The other arguments are
    HotPath.gbuffer_pass'; parts: None, or UR_GBUFFER_PART_RASTER and / or UR_GBUFFER_PART_RESOLVE through ur_forward_pass_parts."""
    rows = h - row0 if rows is None else rows
    assert depth.dtype == torch.float32 and depth.numel() >= w * h
    v, p = _matrix16(view), _matrix16(projection)
    d = raster_draws(commands, command_count, visible, ranges, index_base)
    mask = None
    if mask_draws is not None:
        assert keys64 is not None and keys64.dtype == torch.int64 and keys64.is_contiguous() and keys64.numel() >= w * rows
        mask = C.byref(_lib.GBufferMask(C.pointer(mask_draws), keys64.data_ptr(), _ptr(mask_stats), _ptr(won)))
    table, count = (None, 0) if materials is None else ((materials.table, materials.count) if isinstance(materials, Materials) else materials)
    head = (self._ctx, _lib.fptr(v), _lib.fptr(p), C.byref(d), _ptr(depth), C.byref(targets), w, h, int(row0), int(rows), int(flags), int(key_triangle_bits),
            _ptr(stats))
    tail = (_ptr(table), int(count), mask, C.byref(scene), C.byref(tables))
    if parts is None:
        _lib.check(self._L.ur_forward_pass(*head, *tail), "ur_forward_pass")
    else:
        _lib.check(self._L.ur_forward_pass_parts(*head, int(parts), *tail), "ur_forward_pass_parts")


def _object_id_pass(self, draws, view, projection, depth, w, h, *, object_id=None, keys=None, row0=0, rows=None, flags=0, key_triangle_bits=0, stats=None):
    """ur_object_id_pass: the ObjectId pass of either renderer over the rows [row0, row0 + rows). draws: a raster_draws(...) selection - the
    opaque and the alpha-masked models together - or the commands tensor (every slot); depth: the w x h depth gbuffer_pass(mask_draws=) or
    forward_pass left (depth_prepass' for opaque models), read only. object_id, keys: (rows, w) int32 device tensors, made here when None.
    There is no alpha test: a masked model drawn later than the surface seen through its holes wins there. Returns (object_id, keys)."""
    rows = h - row0 if rows is None else rows
    assert depth.dtype == torch.float32 and depth.numel() >= w * h
    d = draws if isinstance(draws, _lib.RasterDraws) else raster_draws(draws)
    object_id = torch.empty((rows, w), dtype=torch.int32, device=depth.device) if object_id is None else object_id
    keys = torch.empty((rows, w), dtype=torch.int32, device=depth.device) if keys is None else keys
    for t in (object_id, keys):
        assert t.dtype == torch.int32 and t.numel() >= w * rows
    v, p = _matrix16(view), _matrix16(projection)
    _lib.check(self._L.ur_object_id_pass(self._ctx, _lib.fptr(v), _lib.fptr(p), C.byref(d), _ptr(depth), _ptr(object_id), _ptr(keys), w, h, int(row0), int(rows),
                                         int(flags), int(key_triangle_bits), _ptr(stats)), "ur_object_id_pass")
    return object_id, keys


def _object_id_pick(self, draws, view, projection, depth, w, h, points, *, results=None, flags=0, key_triangle_bits=0, stats=None):
    """ur_object_id_pick: what object_id_pass gives at up to lib.UR_PICK_MAX_POINTS texels, from the triangles alone. points: (n, 2) host
    integers (x, y), clamped to the frame by the call. Returns the records as an (n, 4) int32 device tensor - object_id, key, slot (-1 =
    nothing), depth bits per row, lib.PickResult's fields - (`results` when given: 16-byte aligned); nothing is synchronised."""
    pts = np.ascontiguousarray(np.asarray(points, np.int64).reshape(-1, 2).astype(np.uint32))
    n = int(pts.shape[0])
    assert depth.dtype == torch.float32 and depth.numel() >= w * h
    d = draws if isinstance(draws, _lib.RasterDraws) else raster_draws(draws)
    results = torch.empty((n, 4), dtype=torch.int32, device=depth.device) if results is None else results
    assert results.dtype == torch.int32 and results.numel() >= 4 * n
    v, p = _matrix16(view), _matrix16(projection)
    _lib.check(self._L.ur_object_id_pick(self._ctx, _lib.fptr(v), _lib.fptr(p), C.byref(d), _ptr(depth), w, h, int(flags), int(key_triangle_bits),
                                         pts.ctypes.data_as(C.POINTER(C.c_uint32)), n, _ptr(results), _ptr(stats)), "ur_object_id_pick")
    return results


def _transcode_texture(self, data_or_tensor, width: int, height: int, mips: int, format: int):
    """ur_texture_transcode: a chain of BC1 / BC2 / BC3 / BC4 / BC5 / BC7 blocks (bytes or a uint8 array: a DDS file's payload as it lies,
    uploaded here; or a uint8 device tensor that already holds it) is decoded on the device, once, into the RGBA8 chain the sampler is
    fastest on. `format` is one of the ten source codes (lib.UR_TEXTURE_BC*, lib.UR_TEXTURE_SOURCE_*). Returns (the chain as an int32
    device tensor, its lib.Texture2D - UR_TEXTURE_R8G8B8A8_UNORM_SRGB for the _SRGB sources), ready for pack_materials. One launch on the
    context's stream; nothing is synchronised."""
    from . import hostmath
    need = hostmath.texture_chain_bytes(format, width, height, mips)
    if need == 0:
        raise ValueError(f"no source chain: format {format}, {width} x {height}, {mips} mips (71, 72, 74, 75, 77, 78, 80, 83, 98, 99; sizes 1..65535, mips 1..255)")
    blocks = data_or_tensor
    if not isinstance(blocks, torch.Tensor):
        blocks = np.frombuffer(bytes(blocks), np.uint8) if isinstance(blocks, (bytes, bytearray, memoryview)) else np.ascontiguousarray(blocks, np.uint8).reshape(-1)
    have = blocks.numel() if isinstance(blocks, torch.Tensor) else blocks.size
    if have != need:  # (refused before any upload)
        raise ValueError(f"a {width} x {height} chain of {mips} mips in format {format} is {need} bytes, the payload has {have}")
    if not isinstance(blocks, torch.Tensor):
        blocks = to_device(blocks.copy())
    assert blocks.dtype == torch.uint8 and blocks.is_contiguous() and blocks.is_cuda
    out = torch.empty(self._L.ur_texture_transcode_bytes(int(width), int(height), int(mips)) // 4, dtype=torch.int32, device=blocks.device)
    desc = _lib.Texture2D()
    _lib.check(self._L.ur_texture_transcode(self._ctx, int(format), blocks.data_ptr(), int(width), int(height), int(mips), out.data_ptr(), C.byref(desc)),
               "ur_texture_transcode")
    return out, desc


class Mesh:
    """A built mesh on the device: `vertices` (int32 [V, 16]: 64-byte vertices), `indices` (int32 [I]), `sections` (per primitive
    (vertex_offset, index_start, index_count)), `info` (int32 [14]: a lib.MeshInfo record, read with mesh_info once the stream is done) and
    `materials` (per primitive the glTF material index, -1 for none; filled by assets.load_gltf_meshes)."""

    def __init__(self, vertices, indices, sections, info, materials=None):
        self.vertices, self.indices, self.sections, self.info, self.materials = vertices, indices, sections, info, materials

    def mesh_info(self):
        """The lib.MeshInfo record (synchronises: a device-to-host copy)."""
        return _lib.MeshInfo.from_buffer_copy(self.info.cpu().numpy().tobytes())


def _build_mesh(self, buffer, primitives, scratch=None):
    """ur_mesh_build: `buffer` (the glTF .bin as a uint8 device tensor, or bytes / a uint8 array uploaded here) and hostmath.mesh_primitive
    records of one glTF mesh become a Mesh on the device, by the reference's assembly, index expansion and normal / tangent rules
    (DESIGN.md 3.17). Asynchronous on the context's stream; nothing is read back. scratch: a uint8 device tensor of at least the
    layout's scratch_bytes to reuse, else one is allocated."""
    from . import hostmath
    primitives = list(primitives)
    if not isinstance(buffer, torch.Tensor):
        data = np.frombuffer(bytes(buffer), np.uint8) if isinstance(buffer, (bytes, bytearray, memoryview)) else np.ascontiguousarray(buffer, np.uint8).reshape(-1)
        size = data.size
    else:
        assert buffer.dtype == torch.uint8 and buffer.is_contiguous()
        size = buffer.numel()
    layout, sections = hostmath.mesh_layout(primitives, size)  # refuses before anything is uploaded
    if not isinstance(buffer, torch.Tensor):
        buffer = to_device(data.copy())
    assert buffer.is_cuda
    vertices = torch.empty((layout.vertex_count, 16), dtype=torch.int32, device=buffer.device)
    indices = torch.empty(layout.index_count, dtype=torch.int32, device=buffer.device)
    info = torch.empty(C.sizeof(_lib.MeshInfo) // 4, dtype=torch.int32, device=buffer.device)
    if scratch is None:
        scratch = torch.empty(int(layout.scratch_bytes), dtype=torch.uint8, device=buffer.device)
    assert scratch.dtype == torch.uint8 and scratch.is_contiguous() and scratch.numel() >= layout.scratch_bytes
    _lib.check(self._L.ur_mesh_build(self._ctx, buffer.data_ptr(), size, hostmath.mesh_primitive_array(primitives), len(primitives), vertices.data_ptr(),
                                     indices.data_ptr(), scratch.data_ptr(), scratch.numel(), info.data_ptr()), "ur_mesh_build")
    mesh = Mesh(vertices, indices, sections, info)
    mesh._keep = (buffer, scratch)  # (the launches are still in flight)
    return mesh


def mesh_draws(mesh, constants, constants_offset: int = 0, constants_stride: int = 0):
    """pack_draw_commands' dicts for a Mesh: one command per primitive with start_index / index_count from its section, base_vertex 0 (the
    indices already carry the primitive's vertex offset) and stride 64. constants: the device tensor of the draws' constants, primitive k at
    constants_offset + k * constants_stride bytes."""
    return [{"vertices": mesh.vertices, "stride": 64, "indices": mesh.indices, "constants": constants, "constants_offset": constants_offset + k * constants_stride,
             "start_index": start, "index_count": count, "base_vertex": 0} for k, (_, start, count) in enumerate(mesh.sections)]


def mesh_infos(meshes) -> torch.Tensor:
    """The info records of built meshes, stacked on the device as int32 [len(meshes), 14]: ur_scene_build's mesh_infos table. A device copy
    on the current stream; nothing is read back."""
    return torch.stack([m.info for m in meshes]).contiguous()


class SceneTables:
    """The tables of ur_scene_build on the device (include/ur_scene_build.h): `nodes`, `meshes`, `mesh_infos`, `materials` and `draws` as
    device tensors of the records' bytes (any dtype), the counts taken from their sizes; `slot_count` constants records of
    `constants_stride` bytes. The caller keeps them and may patch them between builds (a node's transform, say)."""

    def __init__(self, nodes, meshes, mesh_infos, materials, draws, slot_count=None, constants_stride=608, keep=None):
        def device(t):
            if not isinstance(t, torch.Tensor):
                a = np.ascontiguousarray(t)
                t = to_device(a.view(np.uint8).reshape(-1))
            assert t.is_cuda and t.is_contiguous(), "device tensors must be contiguous CUDA/HIP tensors"
            return t
        self.nodes, self.meshes, self.mesh_infos, self.materials, self.draws = (device(t) for t in (nodes, meshes, mesh_infos, materials, draws))
        size = lambda t, record: t.numel() * t.element_size() // C.sizeof(record)  # noqa: E731
        self.node_count, self.mesh_count = size(self.nodes, _lib.SceneNode), size(self.meshes, _lib.SceneMesh)
        self.material_count, self.draw_count = size(self.materials, _lib.SceneMaterialFactors), size(self.draws, _lib.SceneDraw)
        if size(self.mesh_infos, _lib.MeshInfo) != self.mesh_count:
            raise ValueError(f"{self.mesh_count} mesh records and {size(self.mesh_infos, _lib.MeshInfo)} info records")
        self.slot_count = self.draw_count if slot_count is None else int(slot_count)
        self.constants_stride = int(constants_stride)
        self._keep = keep  # (what the mesh records point at)

    def record(self) -> _lib.SceneBuildTables:
        return _lib.SceneBuildTables(self.nodes.data_ptr(), self.meshes.data_ptr(), self.mesh_infos.data_ptr(), self.materials.data_ptr(), self.draws.data_ptr(),
                                     self.node_count, self.mesh_count, self.material_count, self.draw_count)


class BuiltScene:
    """What ur_scene_build leaves on the device: `bounds` (float32 [D, 2, 4], Frame.resources' bounds and the cull's), `commands` (int32
    [D, 16], what pack_draw_commands + to_device give), `constants` (uint8 [slots, stride]), `centers` (float32 [D, 4]: centre, radius) and
    `summary` (int32 [12]: a lib.SceneBuildSummary, read with scene_summary once the stream is done)."""

    def __init__(self, bounds, commands, constants, centers, summary, scratch):
        self.bounds, self.commands, self.constants, self.centers, self.summary, self.scratch = bounds, commands, constants, centers, summary, scratch

    def scene_summary(self) -> _lib.SceneBuildSummary:
        """The lib.SceneBuildSummary record (synchronises: a device-to-host copy). hostmath.light_view_projection takes its scene_center and
        scene_radius, once at load time, as the reference does."""
        return _lib.SceneBuildSummary.from_buffer_copy(self.summary.cpu().numpy().tobytes())


def _build_scene(self, tables: SceneTables, frame, *, transforms_only: bool = False, out: "BuiltScene | None" = None) -> BuiltScene:
    """ur_scene_build: the tables and the constants template `frame` (a lib.SceneConstants: view, projection, light and shadow fields as
    hostmath fills them) become a BuiltScene: bounds, commands, one constants record per draw, centres and the scene summary, on the
    device. Asynchronous on the context's stream; nothing is read back. out: the BuiltScene to write into (a moving scene's per-frame call),
    else one is allocated. transforms_only: only bounds, centres, World of each draw's record and the summary are rewritten (needs out)."""
    D = tables.draw_count
    if transforms_only and out is None:
        raise ValueError("build_scene: transforms_only rewrites an earlier build: pass it as out")
    if out is None:
        dev = tables.draws.device
        need = int(self._L.ur_scene_build_scratch_bytes(D))
        if need == 0:
            raise ValueError(f"build_scene: {D} draws (1 .. 2^24 - 1)")
        out = BuiltScene(torch.empty((D, 2, 4), dtype=torch.float32, device=dev), torch.empty((D, 16), dtype=torch.int32, device=dev),
                         torch.zeros((tables.slot_count, tables.constants_stride), dtype=torch.uint8, device=dev),
                         torch.empty((D, 4), dtype=torch.float32, device=dev), torch.empty(12, dtype=torch.int32, device=dev),
                         torch.empty(need, dtype=torch.uint8, device=dev))
    assert out.constants.numel() * out.constants.element_size() >= tables.slot_count * tables.constants_stride and out.bounds.numel() * out.bounds.element_size() >= 32 * D
    assert out.commands.numel() * out.commands.element_size() >= 64 * D and (out.centers is None or out.centers.numel() * out.centers.element_size() >= 16 * D)
    outputs = _lib.SceneBuildOutputs(out.bounds.data_ptr(), out.commands.data_ptr(), out.constants.data_ptr(), out.centers.data_ptr() if out.centers is not None else None,
                                     out.summary.data_ptr(), tables.constants_stride, tables.slot_count)
    record = tables.record()
    _lib.check(self._L.ur_scene_build(self._ctx, C.byref(record), C.byref(frame), C.byref(outputs), out.scratch.data_ptr(), out.scratch.numel(),
                                      _lib.UR_SCENE_BUILD_TRANSFORMS_ONLY if transforms_only else 0), "ur_scene_build")
    out._keep = tables  # (the launches are still in flight, and the commands point into the meshes)
    return out


def _build_env_cube(self, payload, format: int, base: int, mips: int, info=None, *, out=None) -> torch.Tensor:
    """ur_env_cube_build: a DDS cube's payload (assets.load_env_cube_dds_source: a uint8 device tensor that holds it, or a uint8 array or
    bytes, uploaded here) is decoded and staged on the device - what stage_env_cube gives for the same cube, to the byte. `format` is
    lib.UR_ENV_SOURCE_*. info: an int32 device tensor whose first word receives the number of reserved-mode BC6H blocks, or None. out: a
    device tensor of ur_env_cube_texels(base, mips) * 8 bytes to build into (an environment that changes while frames run), else one is
    allocated. Returns the staged cube, ready for make_tables. Three launches on the context's stream; nothing is synchronised or read back."""
    need = int(self._L.ur_env_cube_source_bytes(int(format), int(base), int(mips)))
    texels = int(self._L.ur_env_cube_texels(int(base), int(mips)))
    if need == 0 or texels == 0:
        raise ValueError(f"no cube source: format {format}, base size {base}, {mips} mips (10, 95, 96; mips 1..16)")
    src = payload
    if not isinstance(src, torch.Tensor):
        src = np.frombuffer(bytes(src), np.uint8) if isinstance(src, (bytes, bytearray, memoryview)) else np.ascontiguousarray(src, np.uint8).reshape(-1)
    have = src.numel() * src.element_size() if isinstance(src, torch.Tensor) else src.size
    if have != need:  # (refused before any upload)
        raise ValueError(f"a cube of base size {base} with {mips} mips in format {format} is {need} bytes, the payload has {have}")
    if not isinstance(src, torch.Tensor):
        src = to_device(src.copy(), self.device)
    dst = out if out is not None else torch.empty((texels, 4), dtype=torch.int16, device=src.device)
    if dst.numel() * dst.element_size() != 8 * texels:
        raise ValueError(f"a staged cube of base size {base} with {mips} mips is {8 * texels} bytes, out has {dst.numel() * dst.element_size()}")
    _lib.check(self._L.ur_env_cube_build(self._ctx, _ptr(src), need, int(format), int(base), int(mips), _ptr(dst), texels, _ptr(info)), "ur_env_cube_build")
    dst._keep = (src, info)  # (the launches are still in flight)
    return dst


HotPath.build_env_cube = _build_env_cube
def _prefilter_env_cube(self, src, base_size: int, sample_count: int = 1024, *, table=None, out=None, scratch=None) -> torch.Tensor:
    """ur_env_prefilter: the top level of an HDR cube (six RGBA16F faces of a power-of-two edge: a device tensor of 6 * base_size^2 * 8
    bytes, or an array or bytes, uploaded here; assets.load_env_cube_top_level) becomes the prefiltered chain of log2(base_size) + 1 levels
    on the device. Returns the payload, a device tensor in DDS order: what build_env_cube takes as
    lib.UR_ENV_SOURCE_RGBA16F. table: hostmath.env_prefilter_table(base_size, sample_count) on the device (made and uploaded here when
    None); out, scratch: device tensors to write into, else allocated. Nothing is synchronised or read back."""
    base, samples = int(base_size), int(sample_count)
    table_bytes = int(self._L.ur_env_prefilter_table_bytes(base, samples))
    if table_bytes == 0:
        raise ValueError(f"no prefilter: base size {base}, {samples} samples (powers of two, 1..2048 and 16..4096)")
    need, mips = 48 * base * base, base.bit_length()
    dst_bytes, scratch_bytes = int(self._L.ur_env_cube_source_bytes(_lib.UR_ENV_SOURCE_RGBA16F, base, mips)), int(self._L.ur_env_prefilter_scratch_bytes(base))
    if not isinstance(src, torch.Tensor):
        src = np.frombuffer(bytes(src), np.uint8) if isinstance(src, (bytes, bytearray, memoryview)) else np.ascontiguousarray(src).view(np.uint8).reshape(-1)
    have = src.numel() * src.element_size() if isinstance(src, torch.Tensor) else src.size
    if have != need:  # (refused before any upload)
        raise ValueError(f"the top level of a cube of base size {base} is {need} bytes, the source has {have}")
    if not isinstance(src, torch.Tensor):
        src = to_device(src.copy(), self.device)
    if table is None:
        from . import hostmath
        table = to_device(hostmath.env_prefilter_table(base, samples).copy(), self.device)
    dst = out if out is not None else torch.empty((dst_bytes // 8, 4), dtype=torch.int16, device=src.device)
    scratch = scratch if scratch is not None else torch.empty(scratch_bytes, dtype=torch.uint8, device=src.device)
    size = lambda t: t.numel() * t.element_size()  # noqa: E731
    _lib.check(self._L.ur_env_prefilter(self._ctx, _ptr(src), need, base, samples, _ptr(table), size(table), _ptr(dst), size(dst), _ptr(scratch), size(scratch)),
               "ur_env_prefilter")
    dst._keep = (src, table, scratch)  # (the launches are still in flight)
    return dst


def _bake_env_cube(self, src, base_size: int, sample_count: int = 1024, *, table=None, out=None) -> torch.Tensor:
    """prefilter_env_cube chained into build_env_cube: the top level of an HDR cube becomes the staged cube make_tables takes, with
    log2(base_size) + 1 mips, all on the device. out: as in build_env_cube."""
    payload = self.prefilter_env_cube(src, base_size, sample_count, table=table)
    return self.build_env_cube(payload.view(torch.uint8).reshape(-1), _lib.UR_ENV_SOURCE_RGBA16F, int(base_size), int(base_size).bit_length(), out=out)


HotPath.prefilter_env_cube = _prefilter_env_cube
HotPath.bake_env_cube = _bake_env_cube
HotPath.build_scene = _build_scene
HotPath.build_mesh = _build_mesh
HotPath.transcode_texture = _transcode_texture
HotPath.gbuffer_pass = _gbuffer_pass
HotPath.forward_pass = _forward_pass
HotPath.object_id_pass = _object_id_pass
HotPath.object_id_pick = _object_id_pick
HotPath.shadow_map = _shadow_map
HotPath.raster_reserve = _raster_reserve
HotPath.depth_prepass = _depth_prepass


def _frame_set_raster_pass(self, call, keep, record, target, stats, draws, **fields):
    """The three setters below: `call` is the library's ur_frame_set_*_pass, `keep` the attribute that keeps the tensors alive, `draws`
    raster_draws' arguments. Without commands, target and ranges: clear. Else `record`, the pass' empty struct, takes the draws and those of
    `fields` that are not None, a tensor as its address."""
    if draws[0] is None and target is None and draws[3] is None:
        setattr(self, keep, None)
        _lib.check(call(self._f, None), call.__name__)
        return
    d = raster_draws(*draws)
    record.draws = d  # (a copy: the tensors and the ur_draw_ranges it points to are kept through d)
    for field, value in fields.items():
        if value is not None:
            setattr(record, field, value.data_ptr() if isinstance(value, torch.Tensor) else value)
    _lib.check(call(self._f, C.byref(record)), call.__name__)
    setattr(self, keep, (d, target, stats))


def _frame_set_shadow_pass(self, commands=None, shadow_map=None, *, visible=None, ranges=None, index_base=0, stats=None, command_count=None):
    """ur_frame_set_shadow_pass: the draws (as in HotPath.shadow_map), the map and the optional counters of the frames rendered with
    UR_FRAME_SHADOW_PASS (device tensors, kept alive here). No arguments: clear."""
    _frame_set_raster_pass(self, self._L.ur_frame_set_shadow_pass, "_shadow_pass_keep", _lib.FrameShadowPass(), shadow_map, stats,
                           (commands, command_count, visible, ranges, index_base), shadow_map=shadow_map, stats4=stats)


Frame.set_shadow_pass = _frame_set_shadow_pass


def _frame_set_depth_pass(self, commands=None, depth=None, *, visible=None, ranges=None, index_base=0, stats=None, command_count=None, flags=0):
    """ur_frame_set_depth_pass: the draws (as in HotPath.depth_prepass), the depth buffer (the frame's depth_full), the optional counters
    and the ur_depth_prepass flags of the frames rendered with UR_FRAME_DEPTH_PASS (device tensors, kept alive here). No arguments:
    clear."""
    _frame_set_raster_pass(self, self._L.ur_frame_set_depth_pass, "_depth_pass_keep", _lib.FrameDepthPass(), depth, stats,
                           (commands, command_count, visible, ranges, index_base), depth=depth, stats6=stats, flags=int(flags))


Frame.set_depth_pass = _frame_set_depth_pass


def _frame_set_gbuffer_pass(self, commands=None, targets=None, *, visible=None, ranges=None, index_base=0, stats=None, command_count=None, flags=0,
                            key_triangle_bits=0):
    """ur_frame_set_gbuffer_pass: the draws (as in HotPath.gbuffer_pass), the targets (gbuffer_targets(...): the frame's gbuffer_a/b/c and
    lighting_band), the optional counters, the ur_gbuffer_pass flags and the key bits of the frames rendered with UR_FRAME_GBUFFER_PASS
    (device tensors, kept alive here). No arguments: clear."""
    _frame_set_raster_pass(self, self._L.ur_frame_set_gbuffer_pass, "_gbuffer_pass_keep", _lib.FrameGBufferPass(), targets, stats,
                           (commands, command_count, visible, ranges, index_base), targets=targets, stats6=stats, flags=int(flags),
                           key_triangle_bits=int(key_triangle_bits))


Frame.set_gbuffer_pass = _frame_set_gbuffer_pass


def _frame_set_gbuffer_materials(self, materials=None):
    """ur_frame_set_gbuffer_materials: the pack_materials(...) table the "GBuffer" pass of the following frames resolves with
    (ur_gbuffer_pass_materials); None clears it. Kept alive here."""
    self._gbuffer_materials_keep = materials
    if materials is None:
        _lib.check(self._L.ur_frame_set_gbuffer_materials(self._f, None, 0), "ur_frame_set_gbuffer_materials")
    else:
        _lib.check(self._L.ur_frame_set_gbuffer_materials(self._f, _ptr(materials.table), int(materials.count)), "ur_frame_set_gbuffer_materials")


Frame.set_gbuffer_materials = _frame_set_gbuffer_materials


def to_device(a: np.ndarray, device=0) -> torch.Tensor:
    """numpy -> device tensor, reinterpreting unsigned dtypes torch cannot hold (bit patterns are preserved)."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to(f"cuda:{device}")


def to_host(t: torch.Tensor, dtype) -> np.ndarray:
    return t.detach().cpu().numpy().view(dtype)
