"""The asset builds on the device: texture transcode, mesh build, scene build, and the environment cube's build and prefilter."""
from __future__ import annotations

import ctypes as C

import torch

from .. import hostmath
from .. import lib as _lib
from . import tensors
from .tensors import _ptr, nbytes


class Mesh:
    """A built mesh on the device: `vertices` (int32 [V, 16]: 64-byte vertices), `indices` (int32 [I]), `sections` (per primitive
    (vertex_offset, index_start, index_count)), `info` (int32 [14]: a lib.MeshInfo record, read with mesh_info once the stream is done) and
    `materials` (per primitive the glTF material index, -1 for none; filled by assets.load_gltf_meshes)."""

    def __init__(self, vertices, indices, sections, info, materials=None):
        self.vertices, self.indices, self.sections, self.info, self.materials = vertices, indices, sections, info, materials

    def mesh_info(self):
        """The lib.MeshInfo record (synchronises: a device-to-host copy)."""
        return _lib.MeshInfo.from_buffer_copy(self.info.cpu().numpy().tobytes())


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
                t = tensors.to_device(tensors.host_bytes(t, reinterpret=True))
            assert t.is_cuda and t.is_contiguous(), "device tensors must be contiguous CUDA/HIP tensors"
            return t
        self.nodes, self.meshes, self.mesh_infos, self.materials, self.draws = (device(t) for t in (nodes, meshes, mesh_infos, materials, draws))
        size = lambda t, record: nbytes(t) // C.sizeof(record)  # noqa: E731
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


class AssetBuilds:
    """Textures, meshes, scenes and environment cubes built on the context's stream; a host payload is uploaded to the context's device."""

    def transcode_texture(self, data_or_tensor, width: int, height: int, mips: int, format: int):
        """ur_texture_transcode: a chain of BC1 / BC2 / BC3 / BC4 / BC5 / BC7 blocks (bytes or a uint8 array: a DDS file's payload as it lies,
        uploaded here; or a uint8 device tensor that already holds it) is decoded on the device, once, into the RGBA8 chain the sampler is
        fastest on. `format` is one of the ten source codes (lib.UR_TEXTURE_BC*, lib.UR_TEXTURE_SOURCE_*). Returns (the chain as an int32
        device tensor, its lib.Texture2D - UR_TEXTURE_R8G8B8A8_UNORM_SRGB for the _SRGB sources), ready for pack_materials. One launch on the
        context's stream; nothing is synchronised."""
        need = hostmath.texture_chain_bytes(format, width, height, mips)
        if need == 0:
            raise ValueError(f"no source chain: format {format}, {width} x {height}, {mips} mips (71, 72, 74, 75, 77, 78, 80, 83, 98, 99; sizes 1..65535, mips 1..255)")
        with tensors.on_stream(self):
            blocks = tensors.device_bytes(data_or_tensor, need, self.device,
                                          lambda have: f"a {width} x {height} chain of {mips} mips in format {format} is {need} bytes, the payload has {have}")
            assert blocks.dtype == torch.uint8 and blocks.is_contiguous() and blocks.is_cuda
            out = torch.empty(self._L.ur_texture_transcode_bytes(int(width), int(height), int(mips)) // 4, dtype=torch.int32, device=blocks.device)
        desc = _lib.Texture2D()
        _lib.check(self._L.ur_texture_transcode(self._ctx, int(format), blocks.data_ptr(), int(width), int(height), int(mips), out.data_ptr(), C.byref(desc)),
                   "ur_texture_transcode")
        return out, desc

    def build_mesh(self, buffer, primitives, scratch=None):
        """ur_mesh_build: `buffer` (the glTF .bin as a uint8 device tensor, or bytes / a uint8 array uploaded here) and hostmath.mesh_primitive
        records of one glTF mesh become a Mesh on the device, by the reference's assembly, index expansion and normal / tangent rules
        (DESIGN.md 3.17). Asynchronous on the context's stream; nothing is read back. scratch: a uint8 device tensor of at least the
        layout's scratch_bytes to reuse, else one is allocated."""
        primitives = list(primitives)
        tensor = isinstance(buffer, torch.Tensor)
        if tensor:
            assert buffer.dtype == torch.uint8 and buffer.is_contiguous()
        else:
            buffer = tensors.host_bytes(buffer)
        size = buffer.numel() if tensor else buffer.size
        layout, sections = hostmath.mesh_layout(primitives, size)  # (its own refusals, not a size to compare: before anything is uploaded)
        with tensors.on_stream(self):
            if not tensor:
                buffer = tensors.to_device(buffer.copy(), self.device)
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

    def build_scene(self, tables: SceneTables, frame, *, transforms_only: bool = False, out: "BuiltScene | None" = None) -> BuiltScene:
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
            with tensors.on_stream(self):  # (the fill of the constants is queued in front of the build that writes into them)
                out = BuiltScene(torch.empty((D, 2, 4), dtype=torch.float32, device=dev), torch.empty((D, 16), dtype=torch.int32, device=dev),
                                 torch.zeros((tables.slot_count, tables.constants_stride), dtype=torch.uint8, device=dev),
                                 torch.empty((D, 4), dtype=torch.float32, device=dev), torch.empty(12, dtype=torch.int32, device=dev),
                                 torch.empty(need, dtype=torch.uint8, device=dev))
        assert nbytes(out.constants) >= tables.slot_count * tables.constants_stride and nbytes(out.bounds) >= 32 * D
        assert nbytes(out.commands) >= 64 * D and (out.centers is None or nbytes(out.centers) >= 16 * D)
        outputs = _lib.SceneBuildOutputs(out.bounds.data_ptr(), out.commands.data_ptr(), out.constants.data_ptr(), out.centers.data_ptr() if out.centers is not None else None,
                                         out.summary.data_ptr(), tables.constants_stride, tables.slot_count)
        record = tables.record()
        _lib.check(self._L.ur_scene_build(self._ctx, C.byref(record), C.byref(frame), C.byref(outputs), out.scratch.data_ptr(), out.scratch.numel(),
                                          _lib.UR_SCENE_BUILD_TRANSFORMS_ONLY if transforms_only else 0), "ur_scene_build")
        out._keep = tables  # (the launches are still in flight, and the commands point into the meshes)
        return out

    def build_env_cube(self, payload, format: int, base: int, mips: int, info=None, *, out=None) -> torch.Tensor:
        """ur_env_cube_build: a DDS cube's payload (assets.load_env_cube_dds_source: a uint8 device tensor that holds it, or a uint8 array or
        bytes, uploaded here) is decoded and staged on the device - what stage_env_cube gives for the same cube, to the byte. `format` is
        lib.UR_ENV_SOURCE_*. info: an int32 device tensor whose first word receives the number of reserved-mode BC6H blocks, or None. out: a
        device tensor of ur_env_cube_texels(base, mips) * 8 bytes to build into (an environment that changes while frames run), else one is
        allocated. Returns the staged cube, ready for make_tables. Three launches on the context's stream; nothing is synchronised or read back."""
        need = int(self._L.ur_env_cube_source_bytes(int(format), int(base), int(mips)))
        texels = int(self._L.ur_env_cube_texels(int(base), int(mips)))
        if need == 0 or texels == 0:
            raise ValueError(f"no cube source: format {format}, base size {base}, {mips} mips (10, 95, 96; mips 1..16)")
        with tensors.on_stream(self):
            src = tensors.device_bytes(payload, need, self.device,
                                       lambda have: f"a cube of base size {base} with {mips} mips in format {format} is {need} bytes, the payload has {have}")
            dst = out if out is not None else torch.empty((texels, 4), dtype=torch.int16, device=src.device)
        if nbytes(dst) != 8 * texels:
            raise ValueError(f"a staged cube of base size {base} with {mips} mips is {8 * texels} bytes, out has {nbytes(dst)}")
        _lib.check(self._L.ur_env_cube_build(self._ctx, _ptr(src), need, int(format), int(base), int(mips), _ptr(dst), texels, _ptr(info)), "ur_env_cube_build")
        dst._keep = (src, info)  # (the launches are still in flight)
        return dst

    def prefilter_env_cube(self, src, base_size: int, sample_count: int = 1024, *, table=None, out=None, scratch=None) -> torch.Tensor:
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
        with tensors.on_stream(self):
            src = tensors.device_bytes(src, need, self.device, lambda have: f"the top level of a cube of base size {base} is {need} bytes, the source has {have}",
                                       reinterpret=True)
            if table is None:
                table = tensors.to_device(hostmath.env_prefilter_table(base, samples).copy(), self.device)
            dst = out if out is not None else torch.empty((dst_bytes // 8, 4), dtype=torch.int16, device=src.device)
            scratch = scratch if scratch is not None else torch.empty(scratch_bytes, dtype=torch.uint8, device=src.device)
        _lib.check(self._L.ur_env_prefilter(self._ctx, _ptr(src), need, base, samples, _ptr(table), nbytes(table), _ptr(dst), nbytes(dst), _ptr(scratch), nbytes(scratch)),
                   "ur_env_prefilter")
        dst._keep = (src, table, scratch)  # (the launches are still in flight)
        return dst

    def bake_env_cube(self, src, base_size: int, sample_count: int = 1024, *, table=None, out=None) -> torch.Tensor:
        """prefilter_env_cube chained into build_env_cube: the top level of an HDR cube becomes the staged cube make_tables takes, with
        log2(base_size) + 1 mips, all on the device. out: as in build_env_cube."""
        payload = self.prefilter_env_cube(src, base_size, sample_count, table=table)
        return self.build_env_cube(payload.view(torch.uint8).reshape(-1), _lib.UR_ENV_SOURCE_RGBA16F, int(base_size), int(base_size).bit_length(), out=out)
