"""Row-band frames with the post exchange (UR_FRAME_POST_EXCHANGE), for tests/test_gpu_post_band.py (virtual ranks in one process)
and tests/test_gpu_post_band_multirank.py (one fresh process per rank, started by tests/_spawner.py, all on GPU 0 with gloo).

BandFrame renders rank r's band of the C4 frame (tests/_multirank_worker.c4_inputs, pica_pica's camera and light) through the render
graph; with the flag it stops after the "Post Record" pass, and finish() runs the post passes from the gathered records. The same
class with world 1 and no flag is the unsplit single-rank frame the bands are compared with.

    RANK=r WORLD_SIZE=n MASTER_ADDR=127.0.0.1 MASTER_PORT=p python tests/_post_band_worker.py --out DIR [--width W --height H]

runs SEQUENCE: render -> dist.allgather_post_records -> finish_post -> dist.allgather_rows of the RGBA8 bands, and writes the sha256
of every gathered array (all ranks must agree) and, on rank 0, the arrays.
"""
import argparse
import hashlib
import json
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
ASSETS = ROOT / "tests" / "golden" / "assets"

# (flags beyond TONEMAP, DeltaTime, history texel offset from the target or None) of the frames the multi-rank test runs; the gather
# mode of frame k alternates ring / direct
SEQUENCE = (("AE|CAS", 1 / 60, None), ("AE|CAS|FUSE", 1 / 30, 1.5), ("AE|CAS", 1 / 45, -1.5), ("CAS|FUSE", 1 / 45, None),
            ("AE|CAS|FUSE", 1 / 45, 1.5))


def post_flags(spec: str) -> int:
    from unclerenderer_amd import lib
    names = {"AE": lib.UR_FRAME_AUTO_EXPOSURE, "CAS": lib.UR_FRAME_CAS, "FUSE": lib.UR_FRAME_FUSE_TONEMAP_CAS}
    out = 0
    for n in spec.split("|"):
        out |= names[n]
    return out


class Inputs:
    """The whole frame's inputs on the device, once per process; a band is a view of its rows."""

    def __init__(self, hp, w, h):
        import torch
        from tests._multirank_worker import c4_inputs
        from unclerenderer_amd import assets
        from unclerenderer_amd.hotpath import to_device
        self.w, self.h = w, h
        self.fc, g, depth_full, shadow, self.bounds = c4_inputs(w, h, 0, h)
        env, base, mips, _ = assets.load_env_cube_dds(ASSETS / "output_pmrem.dds")
        lut = assets.load_brdf_lut_dds(ASSETS / "PreintegratedGF.dds")
        self.tables = hp.make_tables(to_device(shadow), hp.stage_env_cube(env, base, mips), base, mips, to_device(lut))
        self.A, self.B, self.C = to_device(g.A), to_device(g.B), to_device(g.C)
        self.depth, self.depth_full, self.hdr0 = to_device(g.depth), to_device(depth_full), to_device(g.hdr)
        torch.cuda.synchronize()


class BandFrame:
    """Rank `rank` of `world` equal row bands, with its own Frame, luminance pair, scratch, HZB and records."""

    def __init__(self, hp, inp: Inputs, rank: int, world: int):
        import torch
        from unclerenderer_amd import dist as urdist
        from unclerenderer_amd import hostmath, synth
        from unclerenderer_amd.hotpath import Frame, HzbLayout, post_record_bytes, to_device
        w, h = inp.w, inp.h
        self.inp, self.rank, self.world = inp, rank, world
        self.plan = plan = urdist.plan_bands(h, world, rank)
        r0, n = plan.row0, plan.rows
        lay = HzbLayout(w, h)
        nb = inp.bounds.shape[0]
        i0, i1 = urdist.plan_instances(nb, world, rank)
        dev = "cuda"
        self.hdr = inp.hdr0[r0:r0 + n].clone()
        self.ldr = torch.zeros((n, w), dtype=torch.int32, device=dev)
        self.scratch = torch.zeros((n, w), dtype=torch.int32, device=dev)
        self.lum = (torch.full((1,), float("nan"), device=dev), torch.full((1,), float("nan"), device=dev))
        self.own = torch.zeros(post_record_bytes(w), dtype=torch.uint8, device=dev)
        self.records = torch.zeros((world, post_record_bytes(w)), dtype=torch.uint8, device=dev)
        self.hzb = torch.zeros(lay.total, dtype=torch.float32, device=dev)
        self.args0 = to_device(synth.indirect_args_initial(nb)[i0:i1])
        self.args = self.args0.clone()
        self.vis = torch.zeros(max(1, i1 - i0), dtype=torch.int32, device=dev)
        self.cnt = torch.zeros(1, dtype=torch.int32, device=dev)
        self.res = Frame.resources(w, h, r0, n, inp.A[r0:r0 + n], inp.B[r0:r0 + n], inp.C[r0:r0 + n], inp.depth[r0:r0 + n], self.hdr,
                                   inp.depth_full, self.hzb, lay, inp.tables, to_device(np.ascontiguousarray(inp.bounds[i0:i1])), self.args,
                                   i1 - i0, i0, self.vis, self.cnt, None, self.ldr)
        self.consts = hostmath.pack_culling_constants(inp.fc.view, inp.fc.proj, i1 - i0, True, lay.count, lay.width, lay.height, False)
        self.frame = Frame(hp, frames_in_flight=3, rank=rank, world_size=world)
        self.frame.set_post_records(self.own, self.records)

    def render(self, post: int, delta_time: float, exchange: bool):
        from unclerenderer_amd import lib
        self.frame.set_post(luminance=self.lum, tonemap_scratch=self.scratch, delta_time=delta_time)
        self.hdr.copy_(self.inp.hdr0[self.plan.row0:self.plan.row0 + self.plan.rows])  # Lighting blends into its target: every frame starts from the pre-fill
        self.args.copy_(self.args0)
        flags = lib.UR_FRAME_DEFAULT | lib.UR_FRAME_FUSE_LIGHTING_SKY | lib.UR_FRAME_TONEMAP | post
        if exchange:
            flags |= lib.UR_FRAME_POST_EXCHANGE
        self.frame.render(self.res, self.consts, self.inp.fc.scene, self.inp.fc.sky, flags)

    def finish(self):
        self.frame.finish_post()

    def close(self):
        self.frame.close()


def bits(t) -> int:
    return int(t.cpu().numpy().view(np.uint32)[0])


def sha(t) -> str:
    return hashlib.sha256(np.ascontiguousarray(t.cpu().numpy()).tobytes()).hexdigest()


def run_single(hp, w, h):
    """The unsplit single-rank frame over SEQUENCE: [(ldr, luminance written)] per frame."""
    import torch
    inp = Inputs(hp, w, h)
    f = BandFrame(hp, inp, 0, 1)
    out, W, target = [], 0, None
    for spec, dt, offset in SEQUENCE:
        if offset is not None:
            f.lum[1 - W].fill_(target + offset)
        f.render(post_flags(spec), dt, exchange=False)
        torch.cuda.synchronize()
        ae = "AE" in spec
        out.append((f.ldr.clone(), f.lum[W].clone() if ae else None))
        if ae:
            target = float(f.lum[W].cpu()[0]) if target is None else target
            W = 1 - W
    f.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    a = ap.parse_args()
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    import torch
    import torch.distributed as dist
    from unclerenderer_amd import dist as urdist
    from unclerenderer_amd.hotpath import HotPath
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    hp = HotPath(0)
    try:
        w, h = a.width, a.height
        f = BandFrame(hp, Inputs(hp, w, h), rank, world)
        out, W, target = {}, 0, None
        for k, (spec, dt, offset) in enumerate(SEQUENCE):
            mode = ("ring", "direct")[k % 2]
            if offset is not None:
                f.lum[1 - W].fill_(target + offset)  # the same history texel on every rank: the histories stay in lockstep on their own
            f.render(post_flags(spec), dt, exchange=True)
            torch.cuda.synchronize()
            # the rank's record (packed by the frame into its own tensor) to every rank, every rank's into `records` in rank order
            urdist.allgather_post_records(f.records, f.own, mode=mode)
            torch.cuda.synchronize()
            f.finish()
            full = torch.zeros((h, w), dtype=torch.int32, device="cuda")
            urdist.allgather_rows(full, f.ldr, mode=mode)
            torch.cuda.synchronize()
            out[f"ldr{k}"] = full
            if "AE" in spec:
                out[f"lum{k}"] = f.lum[W].clone()
                target = float(f.lum[W].cpu()[0]) if target is None else target
                W = 1 - W
        names = [r[0] for r in f.frame.report()]
        f.close()
        digest = {k: sha(v) for k, v in out.items()}
        digest["report"] = names
        Path(a.out).mkdir(parents=True, exist_ok=True)
        (Path(a.out) / f"rank{rank}.json").write_text(json.dumps(digest))
        if rank == 0:
            np.savez(Path(a.out) / "rank0.npz", **{k: v.cpu().numpy() for k, v in out.items()})
        dist.barrier()
    finally:
        hp.close()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
