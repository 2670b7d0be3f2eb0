"""The post chain: Tonemap, TemporalAA, AutoExposure and CAS with their band / halo and record forms, and GpuDebugPrint."""
from __future__ import annotations

import ctypes as C

import torch

from .. import lib as _lib
from .tensors import _ptr


def _tonemap_constants(enable_tonemap, exposure_ev, exposure, gamma):
    return _lib.TonemapConstants(int(enable_tonemap), int(exposure_ev is not None), exposure, gamma)  # EnableAutoExposure: an EV texel is given


def _cas_constants(w, h, sharpness):
    return _lib.CasConstants((C.c_float * 2)(1.0 / w, 1.0 / h), sharpness, 0.0)  # TexelDelta as the pass sets it (DeferredRenderer.cpp:1533)


# ---- the sizes of the row bands' records and of the debug-print buffer (include/ur_hotpath.h) ----

def post_record_bytes(w: int) -> int:
    """Bytes of one rank's post record at width w: its first and last HDR rows and the 1024 AutoExposure tap texels, 8 B each."""
    return int(_lib.load().ur_post_record_bytes(w))


def taa_record_bytes(w: int) -> int:
    """Bytes of one rank's TAA record at width w: its second and second-last current rows and the first and last row of the history
    image it reads, 8 B a texel."""
    return int(_lib.load().ur_taa_record_bytes(w))


def debug_print_buffer_bytes() -> int:
    """Bytes of the debug-print buffer: the entry count, then 4096 entries {x, y, code, color} of 16 bytes."""
    return int(_lib.load().ur_debug_print_buffer_bytes())


def debug_print_buffer(device=0) -> torch.Tensor:
    """A zeroed debug-print buffer as an int32 device tensor: [0] the count, [1 + 4 i : 5 + 4 i] entry i."""
    return torch.zeros(debug_print_buffer_bytes() // 4, dtype=torch.int32, device=f"cuda:{device}")


class PostPasses:
    """Tonemap, TemporalAA, AutoExposure and CAS on the context's stream."""

    post_record_bytes = staticmethod(post_record_bytes)
    taa_record_bytes = staticmethod(taa_record_bytes)

    def tonemap(self, hdr, out_rgba8, w, rows, exposure=1.0, gamma=2.2, enable_tonemap=True, exposure_ev=None):
        """Tonemap pass (Tonemap.hlsl) over a band: RGBA16F -> R8G8B8A8_UNORM."""
        k = _tonemap_constants(enable_tonemap, exposure_ev, exposure, gamma)
        _lib.check(self._L.ur_tonemap(self._ctx, C.byref(k), _ptr(hdr), _ptr(exposure_ev), _ptr(out_rgba8), w, rows), "ur_tonemap")

    def temporal_aa(self, current_frame, history_band, output_band, history_weight, use_history, w, h, row0=0, rows=None):
        """TemporalAA resolve (TemporalAA.hlsl): current = full frame, history/output = band rows [row0,row0+rows)."""
        rows = h - row0 if rows is None else rows
        _lib.check(self._L.ur_temporal_aa(self._ctx, _ptr(current_frame), _ptr(history_band), _ptr(output_band), history_weight, int(use_history), w, h, row0, rows),
                   "ur_temporal_aa")

    def temporal_aa_tonemap(self, current_frame, history_band, history_out_band, ldr_out_band, history_weight, use_history, w, h, row0=0, rows=None,
                            exposure=1.0, gamma=2.2, enable_tonemap=True, exposure_ev=None):
        """temporal_aa() followed by tonemap() of its output band, in one launch (the same bytes in history_out_band and ldr_out_band)."""
        rows = h - row0 if rows is None else rows
        k = _tonemap_constants(enable_tonemap, exposure_ev, exposure, gamma)
        _lib.check(self._L.ur_temporal_aa_tonemap(self._ctx, C.byref(k), _ptr(current_frame), _ptr(history_band), _ptr(history_out_band), _ptr(exposure_ev),
                                                  _ptr(ldr_out_band), history_weight, int(use_history), w, h, row0, rows), "ur_temporal_aa_tonemap")

    def auto_exposure(self, hdr_full, out_ev, w, h, prev_ev=None, use_history=False, delta_time=0.0, speed_up=3.0, speed_down=1.0,
                      key=0.3, ev_min=0.1, ev_max=5.0):
        """AutoExposure (AutoExposure.hlsl) of the full RGBA16F frame: one float (the EV Tonemap applies) into out_ev.
        Defaults: RendererConfig.h:28-32."""
        k = _lib.AutoExposureConstants((C.c_float * 2)(w, h), delta_time, speed_up, speed_down, int(use_history), key, ev_min, ev_max)
        _lib.check(self._L.ur_auto_exposure(self._ctx, C.byref(k), _ptr(hdr_full), w, h, _ptr(prev_ev), _ptr(out_ev)), "ur_auto_exposure")

    def cas(self, ldr_full, out_band, w, h, row0=0, rows=None, sharpness=0.5):
        """CAS (Cas.hlsl) of rows [row0,row0+rows) of the full R8G8B8A8 image into a band-local output."""
        rows = h - row0 if rows is None else rows
        k = _cas_constants(w, h, sharpness)
        _lib.check(self._L.ur_cas(self._ctx, C.byref(k), _ptr(ldr_full), _ptr(out_band), w, h, row0, rows), "ur_cas")

    def tonemap_cas(self, hdr_full, out_band, w, h, row0=0, rows=None, exposure=1.0, gamma=2.2, enable_tonemap=True, exposure_ev=None,
                    sharpness=0.5):
        """Tonemap of the full frame then CAS of the band, in one launch (the same bytes as tonemap() followed by cas())."""
        rows = h - row0 if rows is None else rows
        tk, ck = _tonemap_constants(enable_tonemap, exposure_ev, exposure, gamma), _cas_constants(w, h, sharpness)
        _lib.check(self._L.ur_tonemap_cas(self._ctx, C.byref(tk), C.byref(ck), _ptr(hdr_full), _ptr(exposure_ev), _ptr(out_band), w, h, row0, rows),
                   "ur_tonemap_cas")

    # ---- the post exchange of row bands ----
    def pack_post_record(self, hdr_band, record, w, h, row0, rows):
        """This band's post record (rows [row0,row0+rows) of the w x h frame) into `record` (post_record_bytes(w) bytes)."""
        _lib.check(self._L.ur_pack_post_record(self._ctx, _ptr(hdr_band), w, h, row0, rows, _ptr(record)), "ur_pack_post_record")

    def auto_exposure_records(self, records, n_ranks, out_ev, w, h, prev_ev=None, use_history=False, delta_time=0.0, speed_up=3.0, speed_down=1.0,
                              key=0.3, ev_min=0.1, ev_max=5.0):
        """auto_exposure of the whole frame from n_ranks gathered records (rank order): the same bits."""
        k = _lib.AutoExposureConstants((C.c_float * 2)(w, h), delta_time, speed_up, speed_down, int(use_history), key, ev_min, ev_max)
        _lib.check(self._L.ur_auto_exposure_records(self._ctx, C.byref(k), _ptr(records), n_ranks, w, h, _ptr(prev_ev), _ptr(out_ev)),
                   "ur_auto_exposure_records")

    def tonemap_cas_halo(self, hdr_band, above, below, out_band, w, h, row0, rows, exposure=1.0, gamma=2.2, enable_tonemap=True, exposure_ev=None,
                         sharpness=0.5):
        """tonemap_cas of rows [row0,row0+rows) from the band and the HDR rows above / below it (None at the frame's edges)."""
        tk, ck = _tonemap_constants(enable_tonemap, exposure_ev, exposure, gamma), _cas_constants(w, h, sharpness)
        _lib.check(self._L.ur_tonemap_cas_halo(self._ctx, C.byref(tk), C.byref(ck), _ptr(hdr_band), _ptr(above), _ptr(below), _ptr(exposure_ev),
                                               _ptr(out_band), w, h, row0, rows), "ur_tonemap_cas_halo")

    def cas_halo(self, ldr_band, above, below, out_band, w, h, row0, rows, exposure=1.0, gamma=2.2, enable_tonemap=True, exposure_ev=None,
                 sharpness=0.5):
        """cas of rows [row0,row0+rows) from tonemap()'s band output and the HDR rows above / below it, tonemapped with the same constants."""
        tk, ck = _tonemap_constants(enable_tonemap, exposure_ev, exposure, gamma), _cas_constants(w, h, sharpness)
        _lib.check(self._L.ur_cas_halo(self._ctx, C.byref(tk), C.byref(ck), _ptr(ldr_band), _ptr(above), _ptr(below), _ptr(exposure_ev),
                                       _ptr(out_band), w, h, row0, rows), "ur_cas_halo")

    # ---- TemporalAA on row bands ----
    def pack_taa_record(self, hdr_band, history_read_band, use_history, record, w, h, row0, rows):
        """This band's TAA record into `record` (taa_record_bytes(w) bytes); history_read_band may be None iff not use_history."""
        _lib.check(self._L.ur_pack_taa_record(self._ctx, _ptr(hdr_band), _ptr(history_read_band), int(use_history), w, h, row0, rows, _ptr(record)),
                   "ur_pack_taa_record")

    def temporal_aa_halo(self, current_band, cur_above, cur_below, history_band, output_band, history_weight, use_history, w, h, row0, rows,
                         above2=None, hist_above=None, below2=None, hist_below=None, resolved_above=None, resolved_below=None):
        """temporal_aa of rows [row0,row0+rows) from the band and the current rows above / below it (None at the frame's edges); with
        resolved_above / resolved_below (and above2 / below2, hist_above / hist_below) the launch also resolves the rows around the band."""
        _lib.check(self._L.ur_temporal_aa_halo(self._ctx, _ptr(current_band), _ptr(cur_above), _ptr(cur_below), _ptr(history_band), _ptr(output_band),
                                               _ptr(above2), _ptr(hist_above), _ptr(below2), _ptr(hist_below), _ptr(resolved_above), _ptr(resolved_below),
                                               history_weight, int(use_history), w, h, row0, rows), "ur_temporal_aa_halo")

    def temporal_aa_tonemap_halo(self, current_band, cur_above, cur_below, history_band, history_out_band, ldr_out_band, history_weight, use_history,
                                 w, h, row0, rows, above2=None, hist_above=None, below2=None, hist_below=None, resolved_above=None, resolved_below=None,
                                 exposure=1.0, gamma=2.2, enable_tonemap=True, exposure_ev=None):
        """temporal_aa_halo() followed by tonemap() of its output band, in one launch."""
        k = _tonemap_constants(enable_tonemap, exposure_ev, exposure, gamma)
        _lib.check(self._L.ur_temporal_aa_tonemap_halo(self._ctx, C.byref(k), _ptr(current_band), _ptr(cur_above), _ptr(cur_below), _ptr(history_band),
                                                       _ptr(history_out_band), _ptr(exposure_ev), _ptr(ldr_out_band), _ptr(above2), _ptr(hist_above),
                                                       _ptr(below2), _ptr(hist_below), _ptr(resolved_above), _ptr(resolved_below), history_weight,
                                                       int(use_history), w, h, row0, rows), "ur_temporal_aa_tonemap_halo")


class DebugPrint:
    """GpuDebugPrint: the text buffer's reset, the cull counters' lines, PrintString and the draw."""

    debug_print_buffer_bytes = staticmethod(debug_print_buffer_bytes)

    def debug_print_reset(self, buffer, stats=None):
        """Zero the buffer's count and, when given, the cull's two counters (PrepareGpuDebugPrint)."""
        _lib.check(self._L.ur_debug_print_reset(self._ctx, _ptr(buffer), _ptr(stats)), "ur_debug_print_reset")

    def debug_print_stats(self, stats, buffer):
        """GpuDebugPrintStats.hlsl: "FRUSTUM n" / "OCCLUDE n" from stats[0] / stats[1] appended to the buffer."""
        _lib.check(self._L.ur_debug_print_stats(self._ctx, _ptr(stats), _ptr(buffer)), "ur_debug_print_stats")

    def debug_print_text(self, buffer, x, y, text, color=0xFFFFFFFF):
        """PrintString of `text` (str, encoded latin-1, or bytes) at (x, y): 8 pixels a character, stopping at a zero code."""
        raw = text.encode("latin-1") if isinstance(text, str) else bytes(text)
        _lib.check(self._L.ur_debug_print_text(self._ctx, _ptr(buffer), x, y, color, raw, len(raw)), "ur_debug_print_text")

    def debug_print_draw(self, buffer, glyphs, atlas, ldr, w, h, row0=0, rows=None, first_char=32, char_count=96):
        """GpuDebugPrint.hlsl's draw composited in place on rows [row0,row0+rows) of the w x h R8G8B8A8 image (ldr band-local).
        glyphs: (n, 10) float32 device tensor of ur_debug_glyph records indexed by code; atlas: (atlas_h, atlas_w) uint8 device tensor."""
        rows = h - row0 if rows is None else rows
        assert glyphs.dtype == torch.float32 and glyphs.dim() == 2 and glyphs.shape[1] == 10 and atlas.dtype == torch.uint8 and atlas.dim() == 2
        k = _lib.DebugPrintConstants((C.c_float * 2)(w, h), first_char, char_count)
        _lib.check(self._L.ur_debug_print_draw(self._ctx, C.byref(k), _ptr(glyphs), glyphs.shape[0], _ptr(atlas), atlas.shape[1], atlas.shape[0],
                                               _ptr(buffer), _ptr(ldr), w, h, row0, rows), "ur_debug_print_draw")
