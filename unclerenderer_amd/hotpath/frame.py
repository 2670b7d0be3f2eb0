"""The render-graph-driven frame (csrc/frame): its resources, its render call and every setter of what the following frames use."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .. import lib as _lib
from .context import HzbLayout, _host_draw_offsets, cull_view, cull_views_array, draw_ranges
from .raster import raster_draws
from . import tensors
from .tensors import _ptr


def _address(t):
    return t.data_ptr() if t is not None else None


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
        dp = _address
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
        p = _lib.FramePost((C.c_void_p * 2)(_address(luminance[0]), _address(luminance[1])), _address(tonemap_scratch), delta_time, tonemap_exposure,
                           tonemap_gamma, ae_key, ae_min, ae_max, ae_speed_up, ae_speed_down, cas_sharpness)
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
        ptrs = (C.c_void_p * len(history))(*[_address(t) for t in history])
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
            with tensors.on_stream(self._hp):
                offsets = _host_draw_offsets(offsets, command_count)
        dr = draw_ranges(offsets, commands, counts)
        self._draws_keep = dr
        _lib.check(self._L.ur_frame_set_draw_ranges(self._f, C.byref(dr)), "ur_frame_set_draw_ranges")

    def set_cull_views(self, views=()):
        """ur_frame_set_cull_views: the "GPU Culling" pass of the frames rendered with UR_FRAME_CULL_VIEWS also culls these views
        (cull_view(...) results or dicts of its arguments; kept alive here). No views: clear."""
        with tensors.on_stream(self._hp):  # (a view's host draw offsets are uploaded by cull_view)
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

    def set_debug_print(self, buffer=None, glyphs=None, atlas=None, first_char=32, char_count=96):
        """ur_frame_set_debug_print: the text buffer and font (device tensors as in HotPath.debug_print_draw, kept alive here) of the frames
        rendered with UR_FRAME_DEBUG_PRINT. No arguments: clear."""
        if buffer is None and glyphs is None and atlas is None:
            self._debug_print_keep = None
            _lib.check(self._L.ur_frame_set_debug_print(self._f, None), "ur_frame_set_debug_print")
            return
        dp = _lib.FrameDebugPrint(_address(buffer), _address(glyphs), glyphs.shape[0] if glyphs is not None else 0, _address(atlas),
                                  atlas.shape[1] if atlas is not None else 0, atlas.shape[0] if atlas is not None else 0, first_char, char_count)
        _lib.check(self._L.ur_frame_set_debug_print(self._f, C.byref(dp)), "ur_frame_set_debug_print")
        self._debug_print_keep = (buffer, glyphs, atlas)

    def set_shadow_pass(self, commands=None, shadow_map=None, *, visible=None, ranges=None, index_base=0, stats=None, command_count=None):
        """ur_frame_set_shadow_pass: the draws (as in HotPath.shadow_map), the map and the optional counters of the frames rendered with
        UR_FRAME_SHADOW_PASS (device tensors, kept alive here). No arguments: clear."""
        _set_raster_pass(self, self._L.ur_frame_set_shadow_pass, "_shadow_pass_keep", _lib.FrameShadowPass(), shadow_map, stats,
                         (commands, command_count, visible, ranges, index_base), shadow_map=shadow_map, stats4=stats)

    def set_depth_pass(self, commands=None, depth=None, *, visible=None, ranges=None, index_base=0, stats=None, command_count=None, flags=0):
        """ur_frame_set_depth_pass: the draws (as in HotPath.depth_prepass), the depth buffer (the frame's depth_full), the optional counters
        and the ur_depth_prepass flags of the frames rendered with UR_FRAME_DEPTH_PASS (device tensors, kept alive here). No arguments:
        clear."""
        _set_raster_pass(self, self._L.ur_frame_set_depth_pass, "_depth_pass_keep", _lib.FrameDepthPass(), depth, stats,
                         (commands, command_count, visible, ranges, index_base), depth=depth, stats6=stats, flags=int(flags))

    def set_gbuffer_pass(self, commands=None, targets=None, *, visible=None, ranges=None, index_base=0, stats=None, command_count=None, flags=0,
                         key_triangle_bits=0):
        """ur_frame_set_gbuffer_pass: the draws (as in HotPath.gbuffer_pass), the targets (gbuffer_targets(...): the frame's gbuffer_a/b/c and
        lighting_band), the optional counters, the ur_gbuffer_pass flags and the key bits of the frames rendered with UR_FRAME_GBUFFER_PASS
        (device tensors, kept alive here). No arguments: clear."""
        _set_raster_pass(self, self._L.ur_frame_set_gbuffer_pass, "_gbuffer_pass_keep", _lib.FrameGBufferPass(), targets, stats,
                         (commands, command_count, visible, ranges, index_base), targets=targets, stats6=stats, flags=int(flags),
                         key_triangle_bits=int(key_triangle_bits))

    def set_gbuffer_materials(self, materials=None):
        """ur_frame_set_gbuffer_materials: the pack_materials(...) table the "GBuffer" pass of the following frames resolves with
        (ur_gbuffer_pass_materials); None clears it. Kept alive here."""
        self._gbuffer_materials_keep = materials
        if materials is None:
            _lib.check(self._L.ur_frame_set_gbuffer_materials(self._f, None, 0), "ur_frame_set_gbuffer_materials")
        else:
            _lib.check(self._L.ur_frame_set_gbuffer_materials(self._f, _ptr(materials.table), int(materials.count)), "ur_frame_set_gbuffer_materials")

    def report(self):
        """[(pass name, culled, transitions)] of the last executed graph."""
        return [(f[0], f[1] == "1", int(f[2])) for f in _lines(self._L.ur_frame_report, self._f)]

    def report_async(self):
        """[(pass name, ran on the async-compute stream, cross-stream waits)] of the last executed graph."""
        return [(f[0], f[3] == "1", int(f[4])) for f in _lines(self._L.ur_frame_report, self._f)]

    def timing_stats(self):
        return [tuple(fields) for fields in _lines(self._L.ur_rg_timing_stats)]


def _lines(call, *args):
    """The "|"-separated fields of each line of a text the library writes: call(*args, NULL, 0) gives its size, call(*args, buffer, size) it."""
    n = call(*args, None, 0)
    buf = C.create_string_buffer(n)
    call(*args, buf, n)
    return [line.split("|") for line in buf.value.decode().splitlines()]


def _set_raster_pass(frame, call, keep, record, target, stats, draws, **fields):
    """The three raster-pass setters: `call` is the library's ur_frame_set_*_pass, `keep` the attribute that keeps the tensors alive, `draws`
    raster_draws' arguments. Without commands, target and ranges: clear. Else `record`, the pass' empty struct, takes the draws and those of
    `fields` that are not None, a tensor as its address."""
    if draws[0] is None and target is None and draws[3] is None:
        setattr(frame, keep, None)
        _lib.check(call(frame._f, None), call.__name__)
        return
    d = raster_draws(*draws)
    record.draws = d  # (a copy: the tensors and the ur_draw_ranges it points to are kept through d)
    for field, value in fields.items():
        if value is not None:
            setattr(record, field, value.data_ptr() if isinstance(value, torch.Tensor) else value)
    _lib.check(call(frame._f, C.byref(record)), call.__name__)
    setattr(frame, keep, (d, target, stats))
