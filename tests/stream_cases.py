"""The cases of the stream tests (tests/_stream_worker.py runs them, tests/test_gpu_streams.py asserts their records).

A case is one call - or one short chain of calls - of the binding, at the smallest shapes at which it can go wrong. Its inputs that live on
the device come from host(seed) (REAL is what the outputs are compared on, DECOY another valid input of the same shapes: what a launch that
ran ahead of its stream reads); outputs() names the buffers the call writes into, which arrive full of 0xA5; call() makes the call on the
context it is given and returns every buffer to compare, the caller's and the wrapper's own. Nothing here synchronises or picks a stream:
that is the worker's business.

FAMILIES is the static list of names: a family is one worker process. NOT_ASYNC names the cases whose call uploads a host payload itself
and so may wait for the context's stream; every other case must return while its stream is still held."""
from __future__ import annotations

import numpy as np

REAL, DECOY = 1, 2
# what a case's own host code or a comparison raises: the worker records it and goes on (a HIP error is a RuntimeError: it stops)
HOST_ERRORS = (AssertionError, AttributeError, ImportError, IndexError, KeyError, NotImplementedError, TypeError, ValueError)

FAMILIES = {
    "visibility": ("build_hzb", "cull_hzb_1000", "cull_draws_4097", "cull_views_4097", "defer_tail_1", "defer_tail_2"),
    "lighting": ("lighting_streaming", "lighting_sky_streaming", "lighting_sky_per_tile", "lighting_sky_band", "lighting_sky_balanced"),
    "post": ("tonemap[130x9]", "tonemap[515x67]", "temporal_aa[130x9]", "temporal_aa[515x67]", "temporal_aa_tonemap[130x9]",
             "temporal_aa_tonemap[515x67]", "temporal_aa_tonemap_in_place[515x67]", "auto_exposure_twice[130x9]", "auto_exposure_twice[515x67]",
             "cas[130x9]", "cas[515x67]", "tonemap_cas[130x9]", "tonemap_cas[515x67]", "debug_print"),
    "raster": tuple(f"{name}[{queue}]" for name in ("shadow_map", "depth_prepass", "gbuffer_pass", "gbuffer_materials", "gbuffer_masked", "forward_pass",
                                                    "object_id_pass", "object_id_pick", "gbuffer_strip") for queue in ("queue", "no queue")),
    "builds": ("transcode_bc1", "transcode_bc7", "transcode_bc7_bytes", "build_mesh_fans", "build_mesh_duck", "build_mesh_fans_bytes", "build_scene",
               "build_scene_transforms_only", "build_env_cube_sf16", "build_env_cube_sf16_bytes", "prefilter_env_cube", "prefilter_env_cube_own_table",
               "bake_env_cube", "panorama_to_cube", "panorama_to_cube_bytes", "sky_to_cube", "brdf_lut", "bake_sky", "bake_panorama", "load_gltf_meshes"),
    "frame": ("frame_default", "frame_fused_riding_hzb", "frame_post_taa", "frame_post_taa_async", "frame_async_long_lane", "two_contexts"),
}

# the wrappers that upload a host payload themselves: the upload is a synchronous copy behind whatever the context's stream holds
# (bake_sky and bake_panorama have no table argument: their prefilter step makes and uploads its table, as prefilter_env_cube(table=None) does)
NOT_ASYNC = ("transcode_bc7_bytes", "build_mesh_fans_bytes", "build_env_cube_sf16_bytes", "prefilter_env_cube_own_table", "panorama_to_cube_bytes",
             "brdf_lut", "bake_sky", "bake_panorama", "load_gltf_meshes")


class Case:
    """host(seed) -> {name: array}; outputs() -> {name: (shape, torch dtype name)}; prepare(hp, up) -> whatever call() needs beside the
    buffers (made once per context, with the context's stream current, and waited for); call(hp, state, buffers) -> {name: tensor}."""
    name = ""

    def host(self, seed):
        return {}

    def outputs(self):
        return {}

    def prepare(self, hp, up):
        return None

    def call(self, hp, state, d):
        raise NotImplementedError

    def canonical(self, name, array, got):
        """The bytes of output `name` with what depends on where a buffer lies taken out (`got`: every returned tensor)."""
        return array

    def host_results(self, got):
        """What the call returned on the host: compared as it is."""
        return None

    def fixed_inputs(self, state):
        """{name: tensor} of the inputs of host() that live in buffers made by prepare() (a raster pass' commands point at them): a probe
        copies into these where it would upload a fresh tensor."""
        return {}


def _lighting_world(w, h):
    from unclerenderer_amd import hostmath, synth
    fc = hostmath.build_frame_constants("sponza", w, h, shadow_size=128, env_mip_count=5)
    return fc, synth.shadow_map_noise(128, 7), synth.env_cube_procedural(16, 5), synth.brdf_lut_procedural(128, 32)


def _tables(hp, up, shadow, env, lut):
    """(the lighting tables, the staged cube made by a synchronous copy in front of everything)."""
    return hp.make_tables(up(shadow), hp.stage_env_cube(env, 16, 5), 16, 5, up(lut))


def _gbuffer(fc, w, h, seed, row0=0, rows=None):
    """Independent texels (synth.gbuffer_iid): every plane of another seed differs, the depth too."""
    from unclerenderer_amd import synth
    g = synth.gbuffer_iid(w, h, seed)
    sl = slice(row0, h if rows is None else row0 + rows)
    return {"A": g.A[sl], "B": g.B[sl], "C": g.C[sl], "depth": g.depth[sl], "hdr": g.hdr[sl]}


# ---- visibility --------------------------------------------------------------------------------------------------------------------

W, H = 128, 72


class BuildHzb(Case):
    name = "build_hzb"

    def host(self, seed):
        from unclerenderer_amd import hostmath
        fc = hostmath.build_frame_constants("sponza", W, H)
        return {"depth": _gbuffer(fc, W, H, seed)["depth"]}

    def outputs(self):
        from unclerenderer_amd.hotpath import HzbLayout
        return {"hzb": ((HzbLayout(W, H).total,), "float32")}

    def prepare(self, hp, up):
        from unclerenderer_amd.hotpath import HzbLayout
        return HzbLayout(W, H)

    def call(self, hp, lay, d):
        hp.build_hzb(d["depth"], d["hzb"], lay)
        return {"hzb": d["hzb"]}


class Cull(Case):
    """cull_indirect_args of n instances against a built HZB: the argument words, the visible list, the count and the stats; with `draws`
    the compacted commands and the counts of three ranges; with `views` two extra frustum views, each with a mask, a list and a count."""

    def __init__(self, name, n, draws=False, views=False):
        self.name, self.n, self.draws, self.views = name, n, draws, views

    def host(self, seed):
        from tests.test_gpu_cull_draws import _commands
        from unclerenderer_amd import hostmath, synth
        fc = hostmath.build_frame_constants("sponza", W, H)
        return {"bounds": synth.instances_random(self.n, 40 + seed, center=fc.camera_position, box=80.0), "args": _commands(self.n, 50 + seed)}

    def outputs(self):
        n = self.n
        out = {"stats": ((2,), "int32"), "visible_idx": ((n,), "int32"), "visible_count": ((1,), "int32")}
        if self.draws:
            out.update(draw_commands=((n * 16,), "int32"), draw_counts=((3,), "int32"))
        for k in range(2 if self.views else 0):
            out.update({f"mask{k}": (((n + 31) // 32,), "int32"), f"list{k}": ((n,), "int32"), f"count{k}": ((1,), "int32")})
        return out

    def prepare(self, hp, up):
        import torch
        from tests.test_gpu_cull_views import _view_planes
        from unclerenderer_amd import hostmath, synth
        from unclerenderer_amd.hotpath import HzbLayout
        fc = hostmath.build_frame_constants("sponza", W, H)
        lay = HzbLayout(W, H)
        hzb = torch.zeros(lay.total, device="cuda")
        hp.build_hzb(up(synth.gbuffer_scene(fc.view, fc.proj, fc.camera_position, W, H, 3).depth), hzb, lay)  # (a scene's depth: some occluded, some not)
        consts = hostmath.pack_culling_constants(fc.view, fc.proj, self.n, True, lay.count, lay.width, lay.height, True)
        offsets = up(np.array([0, self.n // 3, self.n // 3, self.n], np.uint32)) if self.draws else None  # (the middle range is empty)
        return lay, hzb, consts, offsets, _view_planes(fc, consts)[1:3]

    def call(self, hp, state, d):
        lay, hzb, consts, offsets, planes = state
        kw = {}
        if self.draws:
            kw.update(draw_offsets=offsets, draw_commands=d["draw_commands"], draw_counts=d["draw_counts"])
        if self.views:
            kw["views"] = [dict(planes=planes[k], mask=d[f"mask{k}"], visible_idx=d[f"list{k}"], visible_count=d[f"count{k}"]) for k in range(2)]
        hp.cull_indirect_args(consts, d["bounds"], hzb, lay, d["args"], d["stats"], d["visible_idx"], d["visible_count"], **kw)
        return {k: d[k] for k in ("args", *self.outputs())}

    def canonical(self, name, array, got):
        if name in ("visible_idx", "list0", "list1"):  # (the slots behind the count are not written)
            count = {"visible_idx": "visible_count", "list0": "count0", "list1": "count1"}[name]
            n = int(got[count].view(np.uint8).view(np.uint32)[0])
            return array.view(np.uint32)[:min(n, array.size // 4)] if n <= self.n else array
        return array


class DeferTail(Case):
    """defer_hzb_tail(mode), build_hzb, a streaming Lighting+Sky launch that carries what was held back, then flush: the HZB and the HDR."""

    def __init__(self, mode):
        self.name, self.mode = f"defer_tail_{mode}", mode

    def host(self, seed):
        fc, *_ = _lighting_world(W, H)
        return _gbuffer(fc, W, H, seed)

    def outputs(self):
        from unclerenderer_amd.hotpath import HzbLayout
        return {"hzb": ((HzbLayout(W, H).total,), "float32")}

    def prepare(self, hp, up):
        from unclerenderer_amd.hotpath import HzbLayout
        fc, shadow, env, lut = _lighting_world(W, H)
        return fc, _tables(hp, up, shadow, env, lut), HzbLayout(W, H)

    def call(self, hp, state, d):
        fc, tables, lay = state
        hp.defer_hzb_tail(self.mode)
        try:
            hp.build_hzb(d["depth"], d["hzb"], lay)
            hp.deferred_lighting_sky(fc.scene, fc.sky, d["A"], d["B"], d["C"], d["depth"], tables, d["hdr"], W, H)
            hp.flush()
        finally:
            hp.defer_hzb_tail(0)
        return {"hzb": d["hzb"], "hdr": d["hdr"]}


# ---- lighting ----------------------------------------------------------------------------------------------------------------------

class Lighting(Case):
    """deferred_lighting (sky False) or deferred_lighting_sky over rows [row0, row0 + rows) of a w x h frame, the HDR band blended into. A
    width that is a multiple of 16 takes the streaming kernel, another one the per-tile kernel; balanced: run-time tile claims with chunks
    of four tiles (UR_OPT_BALANCE_CHUNK_SHIFT 2), whose claim words the launch clears itself."""

    def __init__(self, name, w, h, sky=True, row0=0, rows=None, balanced=False):
        self.name, self.w, self.h, self.sky, self.row0, self.rows, self.balanced = name, w, h, sky, row0, (h - row0 if rows is None else rows), balanced

    def host(self, seed):
        fc, *_ = _lighting_world(self.w, self.h)
        return _gbuffer(fc, self.w, self.h, seed, self.row0, self.rows)

    def prepare(self, hp, up):
        fc, shadow, env, lut = _lighting_world(self.w, self.h)
        return fc, _tables(hp, up, shadow, env, lut)

    def call(self, hp, state, d):
        from unclerenderer_amd import lib
        fc, tables = state
        before = hp.get_option(lib.UR_OPT_LIGHTING_BALANCE), hp.get_option(lib.UR_OPT_BALANCE_CHUNK_SHIFT)
        if self.balanced:
            hp.set_option(lib.UR_OPT_LIGHTING_BALANCE, 1)
            hp.set_option(lib.UR_OPT_BALANCE_CHUNK_SHIFT, 2)
        try:
            if self.sky:
                hp.deferred_lighting_sky(fc.scene, fc.sky, d["A"], d["B"], d["C"], d["depth"], tables, d["hdr"], self.w, self.h, self.row0, self.rows)
            else:
                hp.deferred_lighting(fc.scene, d["A"], d["B"], d["C"], tables, d["hdr"], self.w, self.h, self.row0, self.rows)
        finally:
            hp.set_option(lib.UR_OPT_LIGHTING_BALANCE, before[0])
            hp.set_option(lib.UR_OPT_BALANCE_CHUNK_SHIFT, before[1])
        return {"hdr": d["hdr"]}


# ---- post --------------------------------------------------------------------------------------------------------------------------

def _hdr_image(seed, w, h):
    rng = np.random.default_rng(seed)
    img = np.zeros((h, w, 4), np.float16)
    img[..., :3] = (rng.random((h, w, 3)) ** 3 * 6.0).astype(np.float16)
    img[..., 3] = 1.0
    return img.view(np.uint16)


class Post(Case):
    """One call of the post chain on a w x h frame. kind: tonemap, temporal_aa, temporal_aa_tonemap (in_place: the history is read and
    written in the same image), auto_exposure_twice (the second call reads the first one's EV as its history), cas, tonemap_cas."""

    def __init__(self, kind, w, h, in_place=False):
        self.kind, self.w, self.h, self.in_place = kind, w, h, in_place
        self.name = f"{kind}{'_in_place' if in_place else ''}[{w}x{h}]"

    def host(self, seed):
        w, h = self.w, self.h
        if self.kind == "cas":
            return {"ldr": np.random.default_rng(60 + seed).integers(0, 2 ** 32, (h, w), dtype=np.uint32)}
        d = {"hdr": _hdr_image(70 + seed, w, h)}
        if self.kind.startswith("temporal_aa"):
            d["history"] = _hdr_image(80 + seed, w, h)
        if self.kind in ("tonemap", "tonemap_cas", "temporal_aa_tonemap"):
            d["ev"] = np.array([0.25 * seed - 0.5], np.float32)
        return d

    def outputs(self):
        w, h = self.w, self.h
        return {"tonemap": {"ldr": ((h, w), "int32")}, "temporal_aa": {"resolved": ((h, w, 4), "float16")},
                "temporal_aa_tonemap": {"ldr": ((h, w), "int32"), **({} if self.in_place else {"resolved": ((h, w, 4), "float16")})},
                "auto_exposure_twice": {"ev0": ((1,), "float32"), "ev1": ((1,), "float32")}, "cas": {"sharp": ((h, w), "int32")},
                "tonemap_cas": {"sharp": ((h, w), "int32")}}[self.kind]

    def call(self, hp, state, d):
        import torch
        w, h = self.w, self.h
        half = lambda t: t.view(torch.float16)  # noqa: E731
        if self.kind == "tonemap":
            hp.tonemap(half(d["hdr"]), d["ldr"], w, h, exposure=0.9, gamma=2.2, exposure_ev=d["ev"])
            return {"ldr": d["ldr"]}
        if self.kind == "temporal_aa":
            hp.temporal_aa(half(d["hdr"]), half(d["history"]), d["resolved"], 0.9, True, w, h)
            return {"resolved": d["resolved"]}
        if self.kind == "temporal_aa_tonemap":
            resolved = half(d["history"]) if self.in_place else d["resolved"]
            hp.temporal_aa_tonemap(half(d["hdr"]), half(d["history"]), resolved, d["ldr"], 0.9, True, w, h, exposure=0.9, exposure_ev=d["ev"])
            return {"resolved": resolved, "ldr": d["ldr"]}
        if self.kind == "auto_exposure_twice":
            hp.auto_exposure(half(d["hdr"]), d["ev0"], w, h)
            hp.auto_exposure(half(d["hdr"]), d["ev1"], w, h, prev_ev=d["ev0"], use_history=True, delta_time=1 / 60)
            return {"ev0": d["ev0"], "ev1": d["ev1"]}
        if self.kind == "cas":
            hp.cas(d["ldr"], d["sharp"], w, h)
            return {"sharp": d["sharp"]}
        hp.tonemap_cas(half(d["hdr"]), d["sharp"], w, h, exposure=0.9, exposure_ev=d["ev"])
        return {"sharp": d["sharp"]}


class DebugPrintCase(Case):
    """The debug print's reset (count word and the cull's counters), the stats lines, a text of more than one launch and the draw over an image."""
    name = "debug_print"

    def host(self, seed):
        from tests import debug_print_cases as K
        from tests import debug_print_ref as R
        return {"image": R.pack_rgba(K.background(seed)), "counters": np.array([2718 + seed, 31415 * seed], np.uint32),
                "buffer": np.full(self._words(), 0x5A5A5A5A, np.uint32), "cleared": np.array([77, 78 + seed], np.uint32)}

    @staticmethod
    def _words():
        from unclerenderer_amd.hotpath import debug_print_buffer_bytes
        return debug_print_buffer_bytes() // 4

    def prepare(self, hp, up):
        import torch
        from tests import debug_print_cases as K
        atlas, glyphs, first, count = K.builtin_font()
        return up(np.ascontiguousarray(glyphs, np.float32)), up(np.ascontiguousarray(atlas)), first, count, K.W, K.H, torch

    def call(self, hp, state, d):
        glyphs, atlas, first, count, w, h, torch = state
        hp.debug_print_reset(d["buffer"], d["cleared"])
        hp.debug_print_stats(d["counters"], d["buffer"])
        hp.debug_print_text(d["buffer"], 3, 40, bytes(32 + (i % 64) for i in range(700)), 0x80FF8040)
        hp.debug_print_draw(d["buffer"], glyphs, atlas, d["image"], w, h, first_char=first, char_count=count)
        return {k: d[k] for k in ("buffer", "cleared", "image")}

    def canonical(self, name, array, got):
        if name == "buffer":  # (reset clears the count word alone: the entries behind the count keep what the buffer held)
            n = int(array.view(np.uint32)[0])
            return array.view(np.uint32)[:1 + 4 * min(n, 4096)]
        return array


# ---- builds ------------------------------------------------------------------------------------------------------------------------

SHAPE = (20, 12, 5)  # levels 10 x 6, 5 x 3 and 2 x 1 have edge blocks and rows of dwords


class Transcode(Case):
    def __init__(self, name, fmt, as_bytes=False):
        self.name, self.fmt, self.as_bytes = name, fmt, as_bytes

    def _chain(self, seed):
        from tests import texture_source_ref as S
        return S.random_chain(self.fmt, *SHAPE, seed=900 + seed)

    def host(self, seed):
        return {} if self.as_bytes else {"blocks": self._chain(seed)}

    def call(self, hp, state, d):
        chain, desc = hp.transcode_texture(self._chain(REAL).tobytes() if self.as_bytes else d["blocks"], *SHAPE, self.fmt)
        return {"chain": chain, "_desc": (desc.width, desc.height, desc.mips, desc.format, desc.texels == chain.data_ptr())}

    def host_results(self, got):
        return list(got["_desc"])


def _mesh(name):
    from tests import mesh_cases as M
    data, prims = M.case(name)
    return np.frombuffer(data, np.uint8), prims, M.host_primitives(prims)


def _mesh_decoy(data, prims):
    """The same buffer with every position scaled by -0.75: the same layout, other vertices, bounds, normals and tangents."""
    a = data.copy()
    for p in prims:
        offset, stride = p["position"][:2]
        at = (offset + stride * np.arange(p["vertex_count"])[:, None] + np.arange(12)[None, :]).reshape(-1)
        a[at] = (a[at].view("<f4") * np.float32(-0.75)).view(np.uint8)
    return a


class BuildMesh(Case):
    """build_mesh with the wrapper's own vertices, indices, info and scratch: `fans` has a segment longer than a workgroup's tile and two
    entries in the long-segment queue, Duck_0 is the loaded fixture."""

    def __init__(self, name, mesh, as_bytes=False):
        self.name, self.mesh, self.as_bytes = name, mesh, as_bytes

    def host(self, seed):
        data, prims, _ = _mesh(self.mesh)
        return {} if self.as_bytes else {"buffer": data.copy() if seed == REAL else _mesh_decoy(data, prims)}

    def call(self, hp, state, d):
        data, _, records = _mesh(self.mesh)
        mesh = hp.build_mesh(data.tobytes() if self.as_bytes else d["buffer"], records)
        return {"vertices": mesh.vertices, "indices": mesh.indices, "info": mesh.info, "_sections": mesh.sections, "_keep": mesh}

    def host_results(self, got):
        return [list(s) for s in got["_sections"]]


class LoadGltf(Case):
    """assets.load_gltf_meshes of the Duck: the .bin uploaded once by the loader and dropped at its return, one build_mesh a mesh."""
    name = "load_gltf_meshes"

    def call(self, hp, state, d):
        from tests import mesh_cases as M
        from unclerenderer_amd import assets
        meshes = assets.load_gltf_meshes(M.ASSETS / "Duck" / "Duck.gltf", hp)
        got = {"_keep": meshes, "_sections": [m.sections for m in meshes]}
        for k, m in enumerate(meshes):
            got.update({f"vertices{k}": m.vertices, f"indices{k}": m.indices, f"info{k}": m.info})
        return got

    def host_results(self, got):
        return [[list(s) for s in sections] for sections in got["_sections"]]


DRAWS = 130  # three workgroups: the finish launch reads the partial sums of the others


class BuildScene(Case):
    """build_scene into a BuiltScene the wrapper makes (its constants zero-filled by torch); transforms: then two nodes are patched in the
    resident table, on the context's stream as the caller must, and the transforms-only form rewrites the same BuiltScene."""

    def __init__(self, name, transforms=False):
        self.name, self.transforms = name, transforms

    def _tables(self, seed):
        from tests import scene_build_ref as R
        return R.seeded_tables(300 + seed, DRAWS)

    def host(self, seed):
        nodes, meshes, infos, materials, draws, _ = self._tables(seed)
        out = {k: np.ascontiguousarray(v).view(np.uint8).reshape(-1) for k, v in dict(nodes=nodes, meshes=meshes, infos=infos, materials=materials, draws=draws).items()}
        if self.transforms:
            nodes = nodes.copy()
            nodes["translate"][0] += np.float32(3)
            nodes["scale"][-1] *= np.float32(-1.5)
            nodes["max_scale"] = np.abs(nodes["scale"]).max(axis=1)
            out["patched"] = np.ascontiguousarray(nodes).view(np.uint8).reshape(-1)
        return out

    def call(self, hp, state, d):
        import torch
        from tests.test_scene_build_ref import frame
        from unclerenderer_amd.hotpath import SceneTables
        slots = self._tables(REAL)[-1]
        tables = SceneTables(d["nodes"], d["meshes"], d["infos"], d["materials"], d["draws"], slot_count=slots, constants_stride=640)
        built = hp.build_scene(tables, frame())
        if self.transforms:
            with torch.cuda.stream(hp.stream):
                d["nodes"].copy_(d["patched"])
            hp.build_scene(tables, frame(), transforms_only=True, out=built)
        return {"bounds": built.bounds, "commands": built.commands, "constants": built.constants, "centers": built.centers, "summary": built.summary,
                "_keep": built}

    def canonical(self, name, array, got):
        if name == "commands":  # (dwords 8, 9: the address of the draw's constants record, taken relative to the constants' own address)
            a = array.view(np.uint32).reshape(-1, 16).copy()
            address = a[:, 8].astype(np.uint64) | (a[:, 9].astype(np.uint64) << np.uint64(32))
            base = np.uint64(got["_constants_address"])
            inside = (address >= base) & (address < base + np.uint64(got["constants"].size))  # (a skipped draw's command has no record)
            relative = np.where(inside, address - base, address)
            a[:, 8], a[:, 9] = relative & np.uint64(0xFFFFFFFF), relative >> np.uint64(32)
            return a
        return array


class EnvCube(Case):
    """build_env_cube of a BC6H SF16 chain (base 16, five levels) into a cube the wrapper makes, with the reserved-mode count."""

    def __init__(self, name, as_bytes=False):
        self.name, self.as_bytes = name, as_bytes

    def _payload(self, seed):
        from tests import env_cube_ref as R
        return R.random_payload(5100 + seed, R.SF16, 16, 5)

    def host(self, seed):
        return {} if self.as_bytes else {"payload": self._payload(seed)}

    def outputs(self):
        return {"info": ((4,), "int32")}

    def call(self, hp, state, d):
        from tests import env_cube_ref as R
        cube = hp.build_env_cube(self._payload(REAL).tobytes() if self.as_bytes else d["payload"], R.SF16, 16, 5, d["info"])
        return {"cube": cube, "info": d["info"]}


BASE, SAMPLES = 16, 64


class Prefilter(Case):
    """prefilter_env_cube (base 16, 64 samples) with the wrapper's own destination and scratch; own_table: the table made and uploaded by
    the wrapper too; bake: bake_env_cube, which drops the prefilter's payload, table and scratch at its return, their launches in flight."""

    def __init__(self, name, own_table=False, bake=False):
        self.name, self.own_table, self.bake = name, own_table, bake

    def host(self, seed):
        from tests import env_prefilter_ref as P
        return {"top": P.random_cube(9100 + seed, BASE)}

    def prepare(self, hp, up):
        from unclerenderer_amd import hostmath
        return None if self.own_table else up(hostmath.env_prefilter_table(BASE, SAMPLES).copy())

    def call(self, hp, table, d):
        if self.bake:
            return {"cube": hp.bake_env_cube(d["top"], BASE, SAMPLES, table=table)}
        return {"payload": hp.prefilter_env_cube(d["top"], BASE, SAMPLES, table=table)}


class Panorama(Case):
    """panorama_to_cube of a 64 x 32 panorama to base 8; bake: bake_panorama, whose three steps each drop the one before."""

    def __init__(self, name, as_bytes=False, bake=False):
        self.name, self.as_bytes, self.bake = name, as_bytes, bake

    def _texels(self, seed):
        from tests import env_panorama_ref as R
        return np.ascontiguousarray(R.random_panorama(700 + seed, 64, 32), np.uint8)

    def host(self, seed):
        return {} if self.as_bytes else {"rgbe": self._texels(seed).reshape(-1)}

    def call(self, hp, state, d):
        from unclerenderer_amd import environment
        if self.bake:
            return {"cube": environment.bake_panorama(hp, d["rgbe"], 64, 32, 8, 16)}
        return {"top": environment.panorama_to_cube(hp, self._texels(REAL).tobytes() if self.as_bytes else d["rgbe"], 64, 32, 8)}


class Sky(Case):
    """sky_to_cube (no device input: the constants travel by value), brdf_lut 32 x 8 with 16 samples (its table uploaded by the wrapper),
    bake_sky base 16 with 64 samples."""

    def __init__(self, name):
        self.name = name

    def call(self, hp, state, d):
        from tests import env_sky_ref as R
        from unclerenderer_amd import environment
        sky = R.sky_constants((0.3, 0.8, -0.5))
        if self.name == "sky_to_cube":
            return {"top": environment.sky_to_cube(hp, sky, BASE, 2)}
        if self.name == "brdf_lut":
            return {"lut": environment.brdf_lut(hp, 32, 8, 16)}
        return {"cube": environment.bake_sky(hp, sky, BASE, SAMPLES)}


# ---- raster ------------------------------------------------------------------------------------------------------------------------

RW, RH = 64, 64  # the smallest of raycast_ref.TARGETS
PICKS = [(32, 32), (20, 40), (63, 0), (5, 5)]


class Raster(Case):
    """One raster pass over the 64 x 64 target, with room for 4096 large work items (queue) or none. The resolving passes run, as in
    every frame, behind a depth_prepass of the same draws in the same call. The draws' buffers are made once per context and the commands
    point at them; the device input a probe replaces is every draw's constants block (the decoy's World moves the draw by 0.3)."""

    def __init__(self, kind, queue):
        self.kind, self.queue = kind, queue
        self.name = f"{kind}[{'queue' if queue else 'no queue'}]"

    def _scene(self):
        from tests import raycast_ref as RC
        from tests import raycast_tex as T
        if self.kind == "shadow_map":
            return RC.shadow_scene(RW, RH)
        textured = {"gbuffer_materials": "textured", "gbuffer_masked": "masked", "forward_pass": "masked", "gbuffer_strip": "textured strip"}
        return T.SCENES[textured[self.kind]](RW, RH) if self.kind in textured else RC.two_draws_scene(RW, RH)

    def host(self, seed):
        from tests import gbuffer_ref as G
        from tests import raycast_tex as T
        out = {}
        for k, dr in enumerate(self._scene().draws):
            c = np.ascontiguousarray(G.as_device_draw(dr).world, np.float32).reshape(-1).copy()
            if seed != REAL:
                c[12] += np.float32(0.3)  # (row-vector convention: World's translation is its last row)
            out[f"c{k}"] = c
        if self.kind == "forward_pass":
            out["hdr"] = T.background(RW, RH)
        return out

    def fixed_inputs(self, state):
        return {f"c{k}": b[2] for k, b in enumerate(state["dd"].buffers)}

    def outputs(self):
        half, word, six = ((RH, RW, 4), "float16"), ((RH, RW), "int32"), ((6,), "int32")
        depth = {"depth": ((RH, RW), "float32"), "depth_stats": six}
        gb = {**depth, "A": half, "B": half, "C": word, "hdr": half, "keys": word, "stats": six}
        mask = {"keys64": ((RH, RW), "int64"), "mask_stats": six, "won": ((1,), "int32")}
        return {"shadow_map": {"map": ((RH, RW), "float32"), "stats": ((4,), "int32")}, "depth_prepass": depth, "gbuffer_pass": {**gb, "object_id": word},
                "gbuffer_strip": gb, "gbuffer_materials": gb, "gbuffer_masked": {**gb, **mask}, "forward_pass": {**depth, "keys": word, "stats": six, **mask},
                "object_id_pass": {**depth, "stats": six}, "object_id_pick": {**depth, "stats": six}}[self.kind]

    def prepare(self, hp, up):
        from tests import forward_gpu, gbuffer_mask_gpu
        from tests import raycast_tex as T
        from tests.gbuffer_gpu import device_draws
        from tests.gbuffer_tex_gpu import device_materials
        sc = self._scene()
        hp.raster_reserve(1 << 12 if self.queue else 0)
        st = {"sc": sc, "dd": device_draws(sc.draws)}
        if hasattr(sc, "mats"):
            st["mats"] = device_materials(T.ref_materials(sc.mats))
            st["sel"] = gbuffer_mask_gpu.Selections(st["dd"], sc.opaque, list(sc.masked))
        if self.kind == "forward_pass":
            st["frame"] = forward_gpu.DeviceFrame(hp, T.scene_frame(sc))
        return st

    def call(self, hp, st, d):
        import torch
        from unclerenderer_amd.hotpath import forward_targets, gbuffer_targets
        sc, dd, kind = st["sc"], st["dd"], self.kind
        for k in d:  # (every output arrives as 0xA5 bytes; the counters are added to)
            if k.endswith("stats") or k == "won":
                with torch.cuda.stream(hp.stream):
                    d[k].zero_()
        if kind == "shadow_map":
            hp.shadow_map(sc.lvp, dd.commands, d["map"], stats=d["stats"])
            return {k: d[k] for k in ("map", "stats")}
        sel = st.get("sel")
        commands, opaque = (sel.call_commands, sel.opaque) if sel is not None else (dd.commands, {})
        hp.depth_prepass(sc.view, sc.proj, commands, d["depth"], stats=d["depth_stats"], **opaque)
        got = {k: d[k] for k in self.outputs()}
        half = lambda k: d[k].view(torch.float16)  # noqa: E731
        if kind == "object_id_pass":
            got["object_id"], got["keys"] = hp.object_id_pass(dd.commands, sc.view, sc.proj, d["depth"], RW, RH, stats=d["stats"])
        elif kind == "object_id_pick":
            got["picked"] = hp.object_id_pick(dd.commands, sc.view, sc.proj, d["depth"], RW, RH, PICKS, stats=d["stats"])
        elif kind == "forward_pass":
            got["hdr"] = d["hdr"]
            mask = dict(mask_draws=sel.mask_draws, keys64=d["keys64"], mask_stats=d["mask_stats"], won=d["won"])
            hp.forward_pass(sc.view, sc.proj, commands, d["depth"], forward_targets(half("hdr"), d["keys"]), RW, RH, scene=st["frame"].scene, tables=st["frame"].tables,
                            stats=d["stats"], materials=st["mats"], **mask, **opaque)
        elif kind != "depth_prepass":
            tg = gbuffer_targets(half("A"), half("B"), d["C"], half("hdr"), d["keys"], d.get("object_id"))
            kw = dict(materials=st["mats"]) if "mats" in st else {}
            if kind == "gbuffer_masked":
                kw.update(mask_draws=sel.mask_draws, keys64=d["keys64"], mask_stats=d["mask_stats"], won=d["won"])
            hp.gbuffer_pass(sc.view, sc.proj, commands, d["depth"], tg, RW, RH, stats=d["stats"], **kw, **opaque)
        return got


def cases(family):
    """{name: Case} of a family, in FAMILIES' order."""
    from tests import bcn_ref
    from tests import texture_source_ref as S
    made = {
        "visibility": lambda: [BuildHzb(), Cull("cull_hzb_1000", 1000), Cull("cull_draws_4097", 4097, draws=True), Cull("cull_views_4097", 4097, views=True),
                               DeferTail(1), DeferTail(2)],
        "lighting": lambda: [Lighting("lighting_streaming", 128, 72, sky=False), Lighting("lighting_sky_streaming", 128, 72),
                             Lighting("lighting_sky_per_tile", 50, 40), Lighting("lighting_sky_band", 128, 72, row0=13, rows=30),
                             Lighting("lighting_sky_balanced", 128, 72, balanced=True)],
        "post": lambda: [Post(kind, w, h) for kind in ("tonemap", "temporal_aa", "temporal_aa_tonemap", "auto_exposure_twice", "cas", "tonemap_cas")
                         for w, h in ((130, 9), (515, 67))] + [Post("temporal_aa_tonemap", 515, 67, in_place=True), DebugPrintCase()],
        "builds": lambda: [Transcode("transcode_bc1", bcn_ref.BC1), Transcode("transcode_bc7", S.BC7), Transcode("transcode_bc7_bytes", S.BC7, as_bytes=True),
                           BuildMesh("build_mesh_fans", "fans"), BuildMesh("build_mesh_duck", "Duck_0"), BuildMesh("build_mesh_fans_bytes", "fans", as_bytes=True),
                           BuildScene("build_scene"), BuildScene("build_scene_transforms_only", transforms=True), EnvCube("build_env_cube_sf16"),
                           EnvCube("build_env_cube_sf16_bytes", as_bytes=True), Prefilter("prefilter_env_cube"),
                           Prefilter("prefilter_env_cube_own_table", own_table=True), Prefilter("bake_env_cube", bake=True), Panorama("panorama_to_cube"),
                           Panorama("panorama_to_cube_bytes", as_bytes=True), Sky("sky_to_cube"), Sky("brdf_lut"), Sky("bake_sky"),
                           Panorama("bake_panorama", bake=True), LoadGltf()],
        "raster": lambda: [Raster(kind, queue) for kind in ("shadow_map", "depth_prepass", "gbuffer_pass", "gbuffer_materials", "gbuffer_masked", "forward_pass",
                                                            "object_id_pass", "object_id_pick", "gbuffer_strip") for queue in (True, False)],
    }[family]()
    by_name = {c.name: c for c in made}
    assert sorted(by_name) == sorted(FAMILIES[family]) and len(by_name) == len(made), "stream_cases.FAMILIES and cases() disagree"
    return {name: by_name[name] for name in FAMILIES[family]}
