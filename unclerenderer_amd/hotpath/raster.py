"""The raster passes (include/ur_raster.h): draw commands and selections, targets, textures and materials, and the ShadowMap,
DepthPrepass, GBuffer, Forward and ObjectId passes with the pick."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .. import hostmath
from .. import lib as _lib
from . import tensors
from .context import draw_ranges
from .tensors import _ptr, nbytes


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
        index_slots = nbytes(i) // 4
        start = int(d.get("start_index", 0))
        row[0], row[1] = va & 0xFFFFFFFF, va >> 32
        row[2] = int(d.get("vertex_bytes", nbytes(v)))
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
        command_count = nbytes(src) // _lib.UR_INDIRECT_COMMAND_STRIDE if src is not None else 0
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


def forward_targets(hdr, keys) -> _lib.ForwardTargets:
    """ur_forward_targets over device tensors of the band (rows x w): hdr float16 (..., 4), keys int32. Keeps them alive."""
    assert hdr.dtype == torch.float16 and hdr.is_contiguous() and keys.dtype == torch.int32 and keys.is_contiguous()
    tg = _lib.ForwardTargets(hdr.data_ptr(), keys.data_ptr())
    tg._keep = (hdr, keys)
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
    buffer = tensors.to_device(np.concatenate([a.reshape(-1) for a in levels]).view(np.uint32))
    desc = _lib.Texture2D(buffer.data_ptr(), w0, h0, len(levels), _lib.UR_TEXTURE_R8G8B8A8_UNORM_SRGB if srgb else _lib.UR_TEXTURE_R8G8B8A8_UNORM, 0)
    return Texture(buffer, desc)


def pack_texture_bc(payload, width: int, height: int, mips: int, format: int) -> Texture:
    """A chain of BC1 / BC3 / BC5 blocks (bytes or a uint8 array: a DDS file's payload as it lies, level 0 first, no padding) becomes one device
    buffer and its descriptor. `format` is one of lib.UR_TEXTURE_BC*; the length must be what hostmath.bc_chain_bytes gives for the chain."""
    need = hostmath.bc_chain_bytes(format, width, height, mips)
    if need == 0:
        raise ValueError(f"no BC chain: format {format}, {width} x {height}, {mips} mips (UR_TEXTURE_BC*, sizes 1..65535, mips 1..255)")
    buffer = tensors.device_bytes(payload, need, 0, lambda have: f"a {width} x {height} chain of {mips} mips in format {format} is {need} bytes, the payload has {have}")
    assert buffer.data_ptr() % 16 == 0  # (torch allocations are aligned far beyond a block's 16 bytes)
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
    return Materials(tensors.to_device(host), len(materials), keep)


def _material_table(materials):
    """(table, count) of gbuffer_pass' and forward_pass' materials argument: a Materials, such a pair, or None."""
    if materials is None:
        return None, 0
    return (materials.table, materials.count) if isinstance(materials, Materials) else materials


def _mask_record(mask_draws, keys64, w, rows, mask_stats, won) -> _lib.GBufferMask:
    assert keys64 is not None and keys64.dtype == torch.int64 and keys64.is_contiguous() and keys64.numel() >= w * rows
    return _lib.GBufferMask(C.pointer(mask_draws), keys64.data_ptr(), _ptr(mask_stats), _ptr(won))


class RasterPasses:
    """ShadowMap, DepthPrepass, GBuffer, Forward and ObjectId on the context's stream."""

    def raster_reserve(self, max_large_work_items: int):
        """ur_raster_reserve: room for that many (triangle, 64 x 64 tile) entries of the large-triangle queue; 0 frees it."""
        _lib.check(self._L.ur_raster_reserve(self._ctx, int(max_large_work_items)), "ur_raster_reserve")

    def shadow_map(self, lvp, commands, shadow_map, *, visible=None, ranges=None, index_base=0, stats=None, command_count=None, size=None):
        """ur_shadow_map: clear shadow_map ((h, w) float32 device tensor, or flat with size=(w, h)) to 1.0 and rasterise the selected draws
        of `commands` (pack_draw_commands, uploaded) under the orthographic light matrix lvp (16 floats, row-major, row-vector
        convention). visible=(visible_idx, visible_count) or ranges=(offsets, commands, counts) select; stats: uint32[4] device tensor,
        added to."""
        w, h = size if size is not None else (int(shadow_map.shape[1]), int(shadow_map.shape[0]))
        assert shadow_map.dtype == torch.float32 and shadow_map.numel() >= w * h
        m = _matrix16(lvp)
        d = raster_draws(commands, command_count, visible, ranges, index_base)
        _lib.check(self._L.ur_shadow_map(self._ctx, _lib.fptr(m), C.byref(d), _ptr(shadow_map), w, h, _ptr(stats)), "ur_shadow_map")

    def depth_prepass(self, view, projection, commands, depth, *, visible=None, ranges=None, index_base=0, stats=None, command_count=None, size=None,
                      flags=0):
        """ur_depth_prepass: clear depth ((h, w) float32 device tensor, or flat with size=(w, h)) to 0.0 and rasterise the selected draws of
        `commands` under the camera's view and projection (16 floats each, row-major, row-vector convention; reverse-Z), keeping the
        per-texel maximum. The selections are HotPath.shadow_map's; stats: uint32[6] device tensor, added to; flags: UR_DEPTH_QUANTIZE_D24."""
        w, h = size if size is not None else (int(depth.shape[1]), int(depth.shape[0]))
        assert depth.dtype == torch.float32 and depth.numel() >= w * h
        v, p = _matrix16(view), _matrix16(projection)
        d = raster_draws(commands, command_count, visible, ranges, index_base)
        _lib.check(self._L.ur_depth_prepass(self._ctx, _lib.fptr(v), _lib.fptr(p), C.byref(d), _ptr(depth), w, h, int(flags), _ptr(stats)), "ur_depth_prepass")

    def gbuffer_pass(self, view, projection, commands, depth, targets, w, h, row0=0, rows=None, *, visible=None, ranges=None, index_base=0, stats=None,
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
        # six entry points, one argument list: [parts], [table, count] of the _materials and _masked forms, [mask] of the _masked ones
        name = "ur_gbuffer_pass" + ("_masked" if mask_draws is not None else "_materials" if materials is not None else "")
        if parts is not None:
            name, args = name + "_parts", args + (int(parts),)
        if mask_draws is not None or materials is not None:
            table, count = _material_table(materials)
            args += (_ptr(table), int(count))
        if mask_draws is not None:
            args += (C.byref(_mask_record(mask_draws, keys64, w, rows, mask_stats, won)),)
        _lib.check(getattr(self._L, name)(*args), name)

    def forward_pass(self, view, projection, commands, depth, targets, w, h, row0=0, rows=None, *, scene, tables, visible=None, ranges=None, index_base=0,
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
        mask = C.byref(_mask_record(mask_draws, keys64, w, rows, mask_stats, won)) if mask_draws is not None else None
        table, count = _material_table(materials)
        head = (self._ctx, _lib.fptr(v), _lib.fptr(p), C.byref(d), _ptr(depth), C.byref(targets), w, h, int(row0), int(rows), int(flags), int(key_triangle_bits),
                _ptr(stats))
        tail = (_ptr(table), int(count), mask, C.byref(scene), C.byref(tables))
        name, part = ("ur_forward_pass", ()) if parts is None else ("ur_forward_pass_parts", (int(parts),))
        _lib.check(getattr(self._L, name)(*head, *part, *tail), name)

    def object_id_pass(self, draws, view, projection, depth, w, h, *, object_id=None, keys=None, row0=0, rows=None, flags=0, key_triangle_bits=0, stats=None):
        """ur_object_id_pass: the ObjectId pass of either renderer over the rows [row0, row0 + rows). draws: a raster_draws(...) selection - the
        opaque and the alpha-masked models together - or the commands tensor (every slot); depth: the w x h depth gbuffer_pass(mask_draws=) or
        forward_pass left (depth_prepass' for opaque models), read only. object_id, keys: (rows, w) int32 device tensors, made here when None.
        There is no alpha test: a masked model drawn later than the surface seen through its holes wins there. Returns (object_id, keys)."""
        rows = h - row0 if rows is None else rows
        assert depth.dtype == torch.float32 and depth.numel() >= w * h
        d = draws if isinstance(draws, _lib.RasterDraws) else raster_draws(draws)
        with tensors.on_stream(self):
            object_id = torch.empty((rows, w), dtype=torch.int32, device=depth.device) if object_id is None else object_id
            keys = torch.empty((rows, w), dtype=torch.int32, device=depth.device) if keys is None else keys
        for t in (object_id, keys):
            assert t.dtype == torch.int32 and t.numel() >= w * rows
        v, p = _matrix16(view), _matrix16(projection)
        _lib.check(self._L.ur_object_id_pass(self._ctx, _lib.fptr(v), _lib.fptr(p), C.byref(d), _ptr(depth), _ptr(object_id), _ptr(keys), w, h, int(row0), int(rows),
                                             int(flags), int(key_triangle_bits), _ptr(stats)), "ur_object_id_pass")
        return object_id, keys

    def object_id_pick(self, draws, view, projection, depth, w, h, points, *, results=None, flags=0, key_triangle_bits=0, stats=None):
        """ur_object_id_pick: what object_id_pass gives at up to lib.UR_PICK_MAX_POINTS texels, from the triangles alone. points: (n, 2) host
        integers (x, y), clamped to the frame by the call. Returns the records as an (n, 4) int32 device tensor - object_id, key, slot (-1 =
        nothing), depth bits per row, lib.PickResult's fields - (`results` when given: 16-byte aligned); nothing is synchronised."""
        pts = np.ascontiguousarray(np.asarray(points, np.int64).reshape(-1, 2).astype(np.uint32))
        n = int(pts.shape[0])
        assert depth.dtype == torch.float32 and depth.numel() >= w * h
        d = draws if isinstance(draws, _lib.RasterDraws) else raster_draws(draws)
        with tensors.on_stream(self):
            results = torch.empty((n, 4), dtype=torch.int32, device=depth.device) if results is None else results
        assert results.dtype == torch.int32 and results.numel() >= 4 * n
        v, p = _matrix16(view), _matrix16(projection)
        _lib.check(self._L.ur_object_id_pick(self._ctx, _lib.fptr(v), _lib.fptr(p), C.byref(d), _ptr(depth), w, h, int(flags), int(key_triangle_bits),
                                             pts.ctypes.data_as(C.POINTER(C.c_uint32)), n, _ptr(results), _ptr(stats)), "ur_object_id_pick")
        return results
