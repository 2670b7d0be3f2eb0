"""Where the binding's wrappers do their own torch work: on a context made with a side stream and called with the default
stream current, every torch.empty, torch.zeros and tensors.to_device a wrapper makes on the caller's behalf happens with the context's
stream as torch's current stream - so the fill or the upload is queued in front of the launches that use it, and torch's allocator orders
the reuse of a buffer the wrapper drops behind them. Nothing is timed and no bytes are compared here (tests/test_gpu_streams.py does that);
the recorders only note torch.cuda.current_stream() at each call.

The list of calls is held to tests/golden/binding_surface.txt and to every module of the package: every HotPath method and every public
function that takes `hp` is either called here, in every form of its optional out= / scratch= / table= / results=, or named in
ALLOCATES_NOTHING - and then its source names none of the three. A wrapper added later cannot slip past."""
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent

# HotPath methods that make no tensor and upload nothing: they pass the caller's buffers on (checked against their source below)
ALLOCATES_NOTHING = {
    "auto_exposure", "auto_exposure_records", "build_hzb", "build_hzb_band", "build_hzb_tail", "cas", "cas_halo", "close", "ctx",
    "debug_print_buffer_bytes", "debug_print_draw", "debug_print_reset", "debug_print_stats", "debug_print_text", "debug_timeline", "defer_hzb_tail",
    "deferred_lighting", "deferred_lighting_sky", "depth_prepass", "flush", "forward_pass", "gbuffer_pass", "get_option", "lighting_schedule", "make_tables",
    "pack_post_record", "pack_taa_record", "post_record_bytes", "raster_reserve", "reserve", "set_option", "shadow_map", "sky_atmosphere", "stream_ceiling",
    "taa_record_bytes", "temporal_aa", "temporal_aa_halo", "temporal_aa_tonemap", "temporal_aa_tonemap_halo", "time_next_lighting", "tonemap", "tonemap_cas",
    "tonemap_cas_halo",
}
TORCH_WORK = re.compile(r"torch\.(empty|zeros|full|ones|tensor)\(|to_device\(|device_bytes\(|cull_view\(|_host_draw_offsets\(")


class _Torch:
    """A module's `torch` with empty and zeros recorded; everything else is torch's."""

    def __init__(self, torch, note):
        self._torch, self._note = torch, note

    def __getattr__(self, name):
        return getattr(self._torch, name)

    def empty(self, *a, **kw):
        self._note("torch.empty")
        return self._torch.empty(*a, **kw)

    def zeros(self, *a, **kw):
        self._note("torch.zeros")
        return self._torch.zeros(*a, **kw)


@pytest.fixture()
def audit(urlib, monkeypatch):
    """(hp on a side stream, the side stream, the list the recorders append (what, stream) to)."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from unclerenderer_amd import environment, hotpath
    side = torch.cuda.Stream()
    hp = hotpath.HotPath(0, side)
    seen = []
    note = lambda what: seen.append((what, torch.cuda.current_stream()))  # noqa: E731
    for module in (hotpath.context, hotpath.builds, hotpath.raster, hotpath.tensors, environment):
        monkeypatch.setattr(module, "torch", _Torch(torch, note))
    upload = hotpath.tensors.to_device

    def to_device(a, device=0):
        note("tensors.to_device")
        return upload(a, device)

    monkeypatch.setattr(hotpath.tensors, "to_device", to_device)
    assert torch.cuda.current_stream() == torch.cuda.default_stream() and side != torch.cuda.default_stream()
    yield hp, side, seen
    torch.cuda.synchronize()
    hp.close()


def _calls(hp):
    """{wrapper: [(form, call, least number of recorded allocations and uploads)]}: the inputs are made here, on the default stream, and
    waited for; the calls are made by the test."""
    import torch
    from tests import env_cube_ref, env_panorama_ref, env_prefilter_ref, env_sky_ref, mesh_cases, raycast_ref, scene_build_ref
    from tests import texture_source_ref as S
    from tests.gbuffer_gpu import device_draws
    from tests.test_scene_build_ref import frame
    from unclerenderer_amd import assets, environment, hostmath, lib, synth
    from unclerenderer_amd.hotpath import Frame, SceneTables, to_device
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).to("cuda")  # noqa: E731  (not the patched upload)
    byte = lambda n: torch.zeros(n, dtype=torch.uint8, device="cuda")  # noqa: E731
    L = lib.load()
    calls = {}

    chain = S.random_chain(S.BC7, 20, 12, 5, seed=1)
    calls["transcode_texture"] = [("bytes", lambda: hp.transcode_texture(chain.tobytes(), 20, 12, 5, S.BC7), 2),
                                  ("tensor", lambda d=dev(chain): hp.transcode_texture(d, 20, 12, 5, S.BC7), 1)]

    data, prims = mesh_cases.case("quad")
    records = mesh_cases.host_primitives(prims)
    layout, _ = hostmath.mesh_layout(records, len(data))
    buffer = dev(np.frombuffer(data, np.uint8))
    calls["build_mesh"] = [("bytes", lambda: hp.build_mesh(data, records), 5), ("tensor", lambda: hp.build_mesh(buffer, records), 4),
                           ("scratch", lambda s=byte(int(layout.scratch_bytes)): hp.build_mesh(buffer, records, scratch=s), 3)]

    box = mesh_cases.ASSETS / "BoxTextured" / "BoxTextured.gltf"  # (one mesh: the .bin's upload, then build_mesh's four tensors)
    calls["load_gltf_meshes"] = [("", lambda: assets.load_gltf_meshes(box, hp), 5)]

    nodes, meshes, infos, materials, draws, slots = scene_build_ref.seeded_tables(5, 65)
    as_bytes = lambda a: dev(np.ascontiguousarray(a).view(np.uint8).reshape(-1))  # noqa: E731
    tables = SceneTables(*(as_bytes(t) for t in (nodes, meshes, infos, materials, draws)), slot_count=slots)
    built = []
    calls["build_scene"] = [("made here", lambda: built.append(hp.build_scene(tables, frame())), 6), ("out", lambda: hp.build_scene(tables, frame(), out=built[0]), 0),
                            ("transforms_only", lambda: hp.build_scene(tables, frame(), transforms_only=True, out=built[0]), 0)]

    payload = env_cube_ref.random_payload(3, env_cube_ref.SF16, 16, 5)
    texels = int(L.ur_env_cube_texels(16, 5))
    cube_out = lambda: torch.zeros((texels, 4), dtype=torch.int16, device="cuda")  # noqa: E731
    calls["build_env_cube"] = [("bytes", lambda: hp.build_env_cube(payload.tobytes(), env_cube_ref.SF16, 16, 5), 2),
                               ("tensor, out", lambda d=dev(payload), o=cube_out(): hp.build_env_cube(d, env_cube_ref.SF16, 16, 5, out=o), 0)]

    top = env_prefilter_ref.random_cube(4, 16)
    table = dev(hostmath.env_prefilter_table(16, 64))
    d_top = dev(top)
    dst_bytes, scratch_bytes = int(L.ur_env_cube_source_bytes(lib.UR_ENV_SOURCE_RGBA16F, 16, 5)), int(L.ur_env_prefilter_scratch_bytes(16))
    calls["prefilter_env_cube"] = [("array, own table", lambda: hp.prefilter_env_cube(top, 16, 64), 4), ("tensor, table", lambda: hp.prefilter_env_cube(d_top, 16, 64, table=table), 2),
                                   ("out, scratch", lambda o=byte(dst_bytes), s=byte(scratch_bytes): hp.prefilter_env_cube(d_top, 16, 64, table=table, out=o, scratch=s), 0)]
    calls["bake_env_cube"] = [("own table", lambda: hp.bake_env_cube(d_top, 16, 64), 4), ("table, out", lambda o=cube_out(): hp.bake_env_cube(d_top, 16, 64, table=table, out=o), 2)]

    sc = raycast_ref.icosphere_scene(64, 64)
    dd = device_draws(sc.draws)
    depth = torch.zeros((64, 64), dtype=torch.float32, device="cuda")
    word = lambda *shape: torch.zeros(shape, dtype=torch.int32, device="cuda")  # noqa: E731
    calls["object_id_pass"] = [("made here", lambda: hp.object_id_pass(dd.commands, sc.view, sc.proj, depth, 64, 64), 2),
                               ("given", lambda a=word(64, 64), b=word(64, 64): hp.object_id_pass(dd.commands, sc.view, sc.proj, depth, 64, 64, object_id=a, keys=b), 0)]
    calls["object_id_pick"] = [("made here", lambda: hp.object_id_pick(dd.commands, sc.view, sc.proj, depth, 64, 64, [(32, 32), (1, 2)]), 1),
                               ("results", lambda r=word(2, 4): hp.object_id_pick(dd.commands, sc.view, sc.proj, depth, 64, 64, [(32, 32), (1, 2)], results=r), 0)]

    calls["stage_env_cube"] = [("", lambda: hp.stage_env_cube(synth.env_cube_procedural(16, 5), 16, 5), 1)]
    calls["draw_offsets_to_device"] = [("", lambda: hp.draw_offsets_to_device([0, 10, 64], 64), 1)]

    n = 64
    fc = hostmath.build_frame_constants("sponza", 128, 72)
    consts = hostmath.pack_culling_constants(fc.view, fc.proj, n, False, 0, 0, 0, False)
    planes = np.ascontiguousarray(consts[:24]).view(np.float32).copy()
    bounds, args = dev(synth.instances_random(n, 5, center=fc.camera_position, box=60.0)), to_device(synth.indirect_args_initial(n))
    ranges = lambda r: dict(draw_commands=word(n * 16), draw_counts=word(r))  # noqa: E731
    calls["cull_indirect_args"] = [
        ("plain", lambda: hp.cull_indirect_args(consts, bounds, None, None, args), 0),
        ("host draw offsets", lambda kw=ranges(2): hp.cull_indirect_args(consts, bounds, None, None, args, draw_offsets=[0, 10, n], **kw), 1),
        ("a view's host draw offsets", lambda kw=ranges(1): hp.cull_indirect_args(consts, bounds, None, None, args, views=[dict(planes=planes, draw_offsets=[0, n], **kw)]), 1)]

    rgbe = np.ascontiguousarray(env_panorama_ref.random_panorama(6, 64, 32), np.uint8).reshape(-1)
    top_out = lambda base: torch.zeros((6, base, base, 4), dtype=torch.int16, device="cuda")  # noqa: E731
    calls["panorama_to_cube"] = [("bytes", lambda: environment.panorama_to_cube(hp, rgbe.tobytes(), 64, 32, 8), 2),
                                 ("tensor, out", lambda d=dev(rgbe), o=top_out(8): environment.panorama_to_cube(hp, d, 64, 32, 8, out=o), 0)]
    calls["bake_panorama"] = [("array", lambda: environment.bake_panorama(hp, rgbe, 64, 32, 8, 16), 6)]
    sky = env_sky_ref.sky_constants((0.3, 0.8, -0.5))
    calls["sky_to_cube"] = [("made here", lambda: environment.sky_to_cube(hp, sky, 16), 1), ("out", lambda o=top_out(16): environment.sky_to_cube(hp, sky, 16, out=o), 0)]
    calls["bake_sky"] = [("", lambda: environment.bake_sky(hp, sky, 16, 64), 5)]
    calls["brdf_lut"] = [("made here", lambda: environment.brdf_lut(hp, 32, 8, 16), 2),
                         ("out", lambda o=torch.zeros((8, 32, 2), dtype=torch.uint16, device="cuda"): environment.brdf_lut(hp, 32, 8, 16, out=o), 1)]

    frames = []

    def with_frame(call):
        def run():
            if not frames:
                frames.append(Frame(hp))
            call(frames[0])
        return run

    calls["Frame.set_draw_ranges"] = [("host offsets", with_frame(lambda f, kw=ranges(2): f.set_draw_ranges([0, 10, n], kw["draw_commands"], kw["draw_counts"])), 1)]
    calls["Frame.set_cull_views"] = [("a view's host draw offsets", with_frame(lambda f, kw=ranges(1): f.set_cull_views([dict(planes=planes, draw_offsets=[0, n], **kw)])), 1)]
    torch.cuda.synchronize()
    return calls, frames


def test_every_wrapper_does_its_torch_work_on_the_contexts_stream(audit):
    import torch
    hp, side, seen = audit
    calls, frames = _calls(hp)
    seen.clear()  # (the inputs' own uploads, on the default stream)
    wrong, too_few = [], []
    try:
        for name, forms in calls.items():
            for form, call, least in forms:
                seen.clear()
                assert torch.cuda.current_stream() == torch.cuda.default_stream()
                call()
                wrong += [f"{name} ({form}): {what} on {stream}" for what, stream in seen if stream != side]
                if len(seen) < least:
                    too_few.append(f"{name} ({form}): {len(seen)} recorded, at least {least} expected: {[w for w, _ in seen]}")
        torch.cuda.synchronize()
    finally:
        for f in frames:
            f.close()
    assert not too_few, "the recorders missed torch work (the audit would be empty):\n" + "\n".join(too_few)
    assert not wrong, "torch work off the context's stream:\n" + "\n".join(wrong)


def _surface_names():
    """The HotPath methods of tests/golden/binding_surface.txt."""
    lines = (ROOT / "tests" / "golden" / "binding_surface.txt").read_text().splitlines()
    return {m.group(1) for m in (re.match(r"HotPath\.(\w+) (method|staticmethod|property)", line) for line in lines) if m}


def test_the_audit_covers_the_surface(urlib):
    """Needs no device: the names alone."""
    import importlib
    import pkgutil

    import unclerenderer_amd
    from unclerenderer_amd import hotpath

    audited = set(_calls_names())
    methods = _surface_names()
    assert len(methods) > 50
    takes_hp = set()  # every public function of every module of the package that has an `hp` parameter, defined in that module
    modules = [m.name for m in pkgutil.walk_packages(unclerenderer_amd.__path__, "unclerenderer_amd.")]
    assert {"unclerenderer_amd.assets", "unclerenderer_amd.environment", "unclerenderer_amd.scene", "unclerenderer_amd.hotpath.builds"} <= set(modules)
    for name in modules:
        module = importlib.import_module(name)
        takes_hp |= {n for n, f in vars(module).items() if inspect.isfunction(f) and f.__module__ == name and not n.startswith("_")
                     and "hp" in inspect.signature(f).parameters and n != "on_stream"}
    assert {"panorama_to_cube", "bake_panorama", "sky_to_cube", "bake_sky", "brdf_lut", "load_gltf_meshes"} <= takes_hp
    missing = sorted((methods | takes_hp) - audited - ALLOCATES_NOTHING)
    assert not missing, f"neither audited nor named in ALLOCATES_NOTHING: {missing}"
    assert not (ALLOCATES_NOTHING & audited) and ALLOCATES_NOTHING <= methods, sorted(ALLOCATES_NOTHING - methods)
    for name in sorted(ALLOCATES_NOTHING):
        raw = inspect.getattr_static(hotpath.HotPath, name)
        f = raw.fget if isinstance(raw, property) else raw.__func__ if isinstance(raw, staticmethod) else raw
        found = TORCH_WORK.search(inspect.getsource(f))
        assert not found, f"HotPath.{name} is named in ALLOCATES_NOTHING and its source has {found.group(0)!r}"


def _calls_names():
    """The wrappers _calls covers, read from its source (it needs a device to run): the keys it assigns."""
    return re.findall(r'calls\["(?:Frame\.)?(\w+)"\] = ', inspect.getsource(_calls))
