"""Row-band frames with TemporalAA through the post exchange (UR_FRAME_TAA_BAND), for tests/test_gpu_taa_band.py (virtual ranks in one
process) and tests/test_gpu_taa_band_multirank.py (one fresh process per rank, started by tests/_spawner.py, all on GPU 0 with gloo).

TaaBandFrame is tests/_post_band_worker.BandFrame with a band-local history ring and the TAA records; the Lighting pre-fill changes with
the frame number, so every frame resolves a different image. With world 1 and no exchange it is the unsplit frame.

    RANK=r WORLD_SIZE=n MASTER_ADDR=127.0.0.1 MASTER_PORT=p python tests/_taa_band_worker.py --out DIR [--width W --height H]

runs SEQUENCE: render -> dist.allgather_post_records + dist.allgather_taa_records (both in flight) -> finish_post -> dist.allgather_rows
of the RGBA8 band and of every ring image, and writes the sha256 of every gathered array and, on rank 0, the arrays.
"""
import argparse
import json
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from tests._post_band_worker import BandFrame, Inputs, sha  # noqa: E402

# (flags beyond TONEMAP, DeltaTime) of the frames the multi-rank test runs
SEQUENCE = (("TAA|AE|CAS", 1 / 60), ("TAA|AE|CAS|FTAA", 1 / 30), ("TAA|AE|CAS|FUSE", 1 / 45))


def taa_flags(spec: str) -> int:
    from unclerenderer_amd import lib
    names = {"AE": lib.UR_FRAME_AUTO_EXPOSURE, "CAS": lib.UR_FRAME_CAS, "FUSE": lib.UR_FRAME_FUSE_TONEMAP_CAS, "TAA": lib.UR_FRAME_TAA,
             "FTAA": lib.UR_FRAME_FUSE_TAA_TONEMAP, "": 0}
    out = 0
    for n in spec.split("|"):
        out |= names[n]
    return out


class TaaBandFrame(BandFrame):
    """Rank `rank` of `world`: BandFrame plus its band of every history image and its TAA records."""

    def __init__(self, hp, inp: Inputs, rank: int, world: int, frames_in_flight: int = 3):
        import torch
        from unclerenderer_amd.hotpath import Frame, taa_record_bytes
        super().__init__(hp, inp, rank, world)
        w, n = inp.w, self.plan.rows
        if frames_in_flight != 3:
            self.frame.close()
            self.frame = Frame(hp, frames_in_flight=frames_in_flight, rank=rank, world_size=world)
            self.frame.set_post_records(self.own, self.records)
        self.ring = [torch.full((n, w, 4), 0x5A5A, dtype=torch.int16, device="cuda") for _ in range(max(1, frames_in_flight))]
        self.taa_own = torch.zeros(taa_record_bytes(w), dtype=torch.uint8, device="cuda")
        self.taa_records = torch.zeros((world, taa_record_bytes(w)), dtype=torch.uint8, device="cuda")
        self.frame.set_taa(self.ring, 0.9)
        self.frame.set_taa_records(self.taa_own, self.taa_records)

    def render_k(self, k: int, post: int, delta_time: float, exchange: bool):
        """Frame number k: the pre-fill of the Lighting target scaled by 1 + k / 4 (Lighting blends into it)."""
        import torch
        from unclerenderer_amd import lib
        r0, n = self.plan.row0, self.plan.rows
        self.frame.set_post(luminance=self.lum, tonemap_scratch=self.scratch, delta_time=delta_time)
        self.hdr.copy_((self.inp.hdr0[r0:r0 + n].view(torch.float16) * (1.0 + 0.25 * (k % 7))).view(torch.int16))
        self.args.copy_(self.args0)
        flags = lib.UR_FRAME_DEFAULT | lib.UR_FRAME_FUSE_LIGHTING_SKY | lib.UR_FRAME_TONEMAP | post
        if exchange:
            flags |= lib.UR_FRAME_POST_EXCHANGE | (lib.UR_FRAME_TAA_BAND if post & lib.UR_FRAME_TAA else 0)
        self.frame.render(self.res, self.consts, self.inp.fc.scene, self.inp.fc.sky, flags)


def run_single(hp, w, h):
    """The unsplit single-rank frame over SEQUENCE: [(ldr, [ring images], (lum0, lum1))] per frame."""
    import torch
    f = TaaBandFrame(hp, Inputs(hp, w, h), 0, 1)
    out = []
    for k, (spec, dt) in enumerate(SEQUENCE):
        f.render_k(k, taa_flags(spec), dt, exchange=False)
        torch.cuda.synchronize()
        out.append((f.ldr.clone(), [t.clone() for t in f.ring], (f.lum[0].clone(), f.lum[1].clone())))
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
        f = TaaBandFrame(hp, Inputs(hp, w, h), rank, world)
        out = {}
        for k, (spec, dt) in enumerate(SEQUENCE):
            mode = ("ring", "direct")[k % 2]
            f.render_k(k, taa_flags(spec), dt, exchange=True)
            torch.cuda.synchronize()
            a_work = urdist.allgather_post_records(f.records, f.own, async_op=True, mode=mode)  # both exchanges in flight together
            b_work = urdist.allgather_taa_records(f.taa_records, f.taa_own, async_op=True, mode=mode)
            a_work.wait()
            b_work.wait()
            torch.cuda.synchronize()
            f.finish()
            full = torch.zeros((h, w), dtype=torch.int32, device="cuda")
            urdist.allgather_rows(full, f.ldr, mode=mode)
            out[f"ldr{k}"] = full
            for s, img in enumerate(f.ring):
                g = torch.zeros((h, w, 4), dtype=torch.int16, device="cuda")
                urdist.allgather_rows(g, img, mode=mode)
                out[f"ring{k}_{s}"] = g
            torch.cuda.synchronize()
            out[f"lum{k}"] = torch.cat([f.lum[0], f.lum[1]]).clone()
        names = [r[0] for r in f.frame.report()]
        nxt = f.frame.taa_next()
        f.close()
        digest = {k: sha(v) for k, v in out.items()}
        digest["report"] = names
        digest["next"] = [nxt["read_slot"], nxt["write_slot"], int(nxt["use_history"])] + nxt["jitter"].view(np.uint32).tolist()
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
