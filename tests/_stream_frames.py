"""The frame family of the stream tests (tests/_stream_worker.py): Frame.render for three frames running on a side-stream
context, probe H in front of each frame, and two contexts on two side streams interleaved from one host thread.

A frame case renders three 128 x 72 frames, a different G-buffer each, into one set of resources: the second frame's cull reads the first
frame's HZB, the TAA ring of two and the luminance pair carry the frames' history. `want` is the same three frames on the default-stream
context, waited for after each; after every frame the HDR image, the LDR image, both ring images, the luminance pair, the cull's words,
list, count and stats and the HZB are compared. With UR_FRAME_ASYNC_COMPUTE the frame forks its async lane from the context's stream and
joins it back by events: waiting for the context's stream alone must be enough.

frame_async_long_lane is the case that holds the join: 2^20 instances with draw ranges and four extra views, each with draw ranges of its
own, make the lane's cull - and the Build HZB queued behind it - outlast the main stream's one fused Lighting+Sky launch, and copies of the HZB, the counts, the stats and
the cull's words are queued on the context's stream right behind the frame, as an engine's next pass would read them. Without the join
those copies run when the main stream's own launch is done, and hold what the frame before left: with the join taken out of a scratch build the
copies behind frame 0 held a stale HZB and stale counts in every run; behind frames 1 and 2 the lane had ended in time."""
import time
import traceback

import numpy as np

from tests import stream_cases as SC

W, H, N = 128, 72, 600
LONG_N, LONG_VIEWS = 1 << 20, 4  # (2^20: what a context's cull workspace holds from its creation on; more would grow it, with a wait for the device)
_HOST = {}
FRAMES = 3
ROUNDS = 8


def frame_flags(name):
    from unclerenderer_amd import lib
    if name == "frame_async_long_lane":
        return lib.UR_FRAME_DEFAULT | lib.UR_FRAME_FUSE_LIGHTING_SKY | lib.UR_FRAME_ASYNC_COMPUTE | lib.UR_FRAME_CULL_VIEWS  # (one launch on the main stream)
    post = lib.UR_FRAME_DEFAULT | lib.UR_FRAME_TONEMAP | lib.UR_FRAME_AUTO_EXPOSURE | lib.UR_FRAME_TAA | lib.UR_FRAME_CAS
    return {"frame_default": lib.UR_FRAME_DEFAULT,
            "frame_fused_riding_hzb": lib.UR_FRAME_DEFAULT | lib.UR_FRAME_FUSE_LIGHTING_SKY | lib.UR_FRAME_HZB_WITH_LIGHTING,
            "frame_post_taa": post, "frame_post_taa_async": post | lib.UR_FRAME_ASYNC_COMPUTE}[name]


class FrameRun:
    """One context's frame and resources; everything is made with the context's stream current and waited for."""

    def __init__(self, torch, hp, upload, long_lane=False):
        from unclerenderer_amd import hostmath, synth
        from unclerenderer_amd.hotpath import Frame, HzbLayout
        self.torch, self.hp, self.long_lane, self.snap = torch, hp, long_lane, {}
        N = self.n = LONG_N if long_lane else globals()["N"]
        if N not in _HOST:  # (computed once: both contexts upload the same arrays)
            fc = hostmath.build_frame_constants("sponza", W, H, shadow_size=128, env_mip_count=5)
            _HOST[N] = synth.instances_random(N, 31, center=fc.camera_position, box=60.0), synth.indirect_args_initial(N)
        with torch.cuda.stream(hp.stream):
            self.fc = hostmath.build_frame_constants("sponza", W, H, shadow_size=128, env_mip_count=5)
            shadow, env, lut = synth.shadow_map_noise(128, 31), synth.env_cube_procedural(16, 5), synth.brdf_lut_procedural(128, 32)
            self.tables = hp.make_tables(upload(shadow), hp.stage_env_cube(env, 16, 5), 16, 5, upload(lut))
            self.lay = HzbLayout(W, H)
            self.bounds = upload(_HOST[N][0])
            self.args0 = upload(_HOST[N][1])
            self.g = []
            for k in range(FRAMES):
                # (the long lane's frames differ in their depth too, so that an HZB left by the frame before shows)
                g = synth.gbuffer_iid(W, H, 31 + k) if long_lane else synth.gbuffer_scene(self.fc.view, self.fc.proj, self.fc.camera_position, W, H, 31 + k)
                self.g.append(tuple(upload(a) for a in (g.A, g.B, g.C, g.depth, g.hdr)))
            word = lambda *shape: torch.zeros(shape, dtype=torch.int32, device="cuda")  # noqa: E731
            self.hzb = torch.zeros(self.lay.total, device="cuda")
            self.args, self.stats, self.vis, self.cnt = self.args0.clone(), word(2), word(N), word(1)
            self.ldr, self.scratch = word(H, W), word(H, W)
            self.ring = [torch.full((H, W, 4), 0x5A5A, dtype=torch.int16, device="cuda") for _ in range(2)]
            self.lum = (torch.full((1,), float("nan"), device="cuda"), torch.full((1,), float("nan"), device="cuda"))
            self.consts = hostmath.pack_culling_constants(self.fc.view, self.fc.proj, 0, False, 0, 0, 0, True)
            self.frame = Frame(hp, frames_in_flight=2)
            self.frame.set_taa(self.ring, 0.9)
            self.frame.set_post(luminance=self.lum, tonemap_scratch=self.scratch, delta_time=1 / 60)
            self.extra = {}
            if long_lane:
                from tests.test_gpu_cull_views import _view_planes
                planes = _view_planes(self.fc, self.consts)[:LONG_VIEWS]  # (the camera's own, the light's, a cascade's, a turned camera's)
                self.extra = {"draw_commands": word(N * 16), "draw_counts": word(1)}
                offsets = upload(np.array([0, N], np.uint32))
                self.frame.set_draw_ranges(offsets, self.extra["draw_commands"], self.extra["draw_counts"])
                views = []
                for v in range(LONG_VIEWS):  # (each view with a mask, a list and draw ranges: 64 bytes written per visible command and view)
                    self.extra.update({f"mask{v}": word((N + 31) // 32), f"list{v}": word(N), f"count{v}": word(1), f"view_commands{v}": word(N * 16),
                                       f"draw_counts{v}": word(1)})
                    views.append(dict(planes=planes[v], mask=self.extra[f"mask{v}"], visible_idx=self.extra[f"list{v}"], visible_count=self.extra[f"count{v}"],
                                      draw_offsets=offsets, draw_commands=self.extra[f"view_commands{v}"], draw_counts=self.extra[f"draw_counts{v}"]))
                self.frame.set_cull_views(views)
        torch.cuda.synchronize()

    def render(self, k, flags):
        """Frame k: the cull's argument words are put back on the context's stream, as the caller of a frame does, then the frame."""
        from unclerenderer_amd.hotpath import Frame
        dA, dB, dC, dD, hdr = self.g[k]
        with self.torch.cuda.stream(self.hp.stream):
            self.args.copy_(self.args0)
        res = Frame.resources(W, H, 0, H, dA, dB, dC, dD, hdr, dD, self.hzb, self.lay, self.tables, self.bounds, self.args, self.n, 0, self.vis, self.cnt, self.stats,
                              tonemap_band=self.ldr)
        self.frame.render(res, self.consts, self.fc.scene, self.fc.sky, flags)
        if self.long_lane:  # (what the next pass on the context's stream would read, queued right behind the frame)
            with self.torch.cuda.stream(self.hp.stream):
                self.snap = {f"behind the frame: {name}": t.clone() for name, t in
                             [("hzb", self.hzb), ("visible_count", self.cnt), ("stats", self.stats), ("draw_counts", self.extra["draw_counts"])]
                             + [(f"{name}{v}", self.extra[f"{name}{v}"]) for v in range(LONG_VIEWS) for name in ("count", "draw_counts")] + [("args", self.args)]}

    def read(self, k):
        """{name: bytes} of everything frame k left, by copies on the current stream."""
        t = {"hdr": self.g[k][4], "ldr": self.ldr, "ring0": self.ring[0], "ring1": self.ring[1], "lum0": self.lum[0], "lum1": self.lum[1], "args": self.args,
             "visible_idx": self.vis, "visible_count": self.cnt, "stats": self.stats, "hzb": self.hzb, **self.snap,
             **{k: v for k, v in self.extra.items() if k.startswith(("count", "draw_counts", "mask"))}}
        out = {name: v.contiguous().view(-1).view(self.torch.uint8).cpu().numpy().tobytes() for name, v in t.items()}
        n = int(np.frombuffer(out["visible_count"], np.uint32)[0])
        out["visible_idx"] = out["visible_idx"][:4 * min(n, self.n)]  # (the slots behind the count are not written)
        return out

    def close(self):
        self.torch.cuda.synchronize()
        self.frame.close()


def run_frames(runner, name):
    torch = runner.torch
    flags = frame_flags(name)
    long_lane = name == "frame_async_long_lane"
    ref = FrameRun(torch, runner.default, runner.upload, long_lane)
    want, call_ms = [], 0.0
    for k in range(FRAMES):
        t0 = time.perf_counter()
        ref.render(k, flags)
        torch.cuda.synchronize()
        call_ms = max(call_ms, (time.perf_counter() - t0) * 1e3)
        want.append(ref.read(k))
    ref.close()
    ms = runner.duration_ms(call_ms)
    side = FrameRun(torch, runner.side, runner.upload, long_lane)
    frames = []
    for k in range(FRAMES):
        torch.cuda.synchronize()
        held = runner.blocker.hold(torch.cuda.default_stream(), ms)
        side.render(k, flags)
        runner.A.synchronize()
        valid = not held.query()
        with torch.cuda.stream(runner.A):
            on_stream = side.read(k)
        torch.cuda.synchronize()
        after = side.read(k)
        frames.append({"valid": valid, "on_stream": runner.differing(on_stream, want[k]), "after_device_wait": runner.differing(after, want[k])})
    side.close()
    ok = all(f["valid"] and not f["on_stream"] and not f["after_device_wait"] for f in frames)
    return {"call_ms": round(call_ms, 3), "blocker_ms": round(ms, 1), "H": {"valid": all(f["valid"] for f in frames), "frames": frames, "ok": ok}, "ok": ok}


def run_two_contexts(runner):
    """HotPath(0, A) runs the lighting cases, HotPath(0, B) the `fans` mesh build and the 4097-instance cull, interleaved for ROUNDS rounds
    with nothing between them; then one wait for the device, and each call's outputs are its own serial `want`."""
    from unclerenderer_amd.hotpath import HotPath
    torch = runner.torch
    on_a = list(SC.cases("lighting").values())
    on_b = [SC.BuildMesh("build_mesh_fans", "fans"), SC.Cull("cull_hzb_4097", 4097)]
    want = {c.name: runner.want(c)[0] for c in on_a + on_b}
    other = HotPath(0, runner.B)
    try:
        plan = []
        for r in range(ROUNDS):
            for hp, case in ((runner.side, on_a[r % len(on_a)]), (other, on_b[r % len(on_b)])):
                st = runner.state(case, hp)
                plan.append((hp, case, st, runner.buffers(case, SC.REAL, st)))
        torch.cuda.synchronize()
        got = [case.call(hp, st, d) for hp, case, st, d in plan]  # (one host thread, no wait anywhere)
        torch.cuda.synchronize()
        bad = []
        for r, ((hp, case, _, _), g) in enumerate(zip(plan, got)):
            bad += [f"round {r // 2}, {case.name} on {'A' if hp is runner.side else 'B'}: {d}" for d in runner.differing(runner.read(case, g), want[case.name])]
    finally:
        torch.cuda.synchronize()
        runner.states = {k: v for k, v in runner.states.items() if k[1] != id(other)}
        other.close()
    return {"rounds": ROUNDS, "differing": bad, "ok": not bad}


def run(runner, records, only=None):
    for name in SC.FAMILIES["frame"]:
        if only in (None, name):
            try:
                records[name] = run_two_contexts(runner) if name == "two_contexts" else run_frames(runner, name)
            except SC.HOST_ERRORS:  # (this file's own host code or a comparison: the next case may run)
                records[name] = {"ok": False, "error": traceback.format_exc()}
            print(name, "ok" if records[name]["ok"] else "FAILED", flush=True)
