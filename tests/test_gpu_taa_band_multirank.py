"""TemporalAA on row bands across real rank processes: two FRESH processes (children of tests/_spawner.py; both on GPU 0 with gloo, as
tests/test_gpu_post_band_multirank.py does) each render their band of the 1920x1080 C4 frame with UR_FRAME_TAA_BAND, all-gather the post
records and the TAA records (both in flight together; ring and direct in turn), run Frame.finish_post and all-gather the RGBA8 band and
their band of every history image. Over tests/_taa_band_worker.SEQUENCE - three frames, unfused, TAA+Tonemap fused, Tonemap+CAS fused -
every rank must end with the single-rank frame's LDR image, ring images and EV, byte for byte."""
import json
import socket
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
WORKER = str(ROOT / "tests" / "_taa_band_worker.py")


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_reproduce_the_single_rank_taa_frames(hotpath, spawn_ranks, tmp_path):
    from tests._taa_band_worker import SEQUENCE, run_single
    world, port = 2, _port()
    envs = [dict(RANK=r, LOCAL_RANK=r, WORLD_SIZE=world, MASTER_ADDR="127.0.0.1", MASTER_PORT=port, HSA_ENABLE_IPC_MODE_LEGACY=0, OMP_NUM_THREADS=4)
            for r in range(world)]
    res = spawn_ranks([sys.executable, WORKER, "--out", str(tmp_path)], envs, timeout=540)
    assert res["rc"] == [0] * world, "rank processes failed:\n" + "\n----\n".join(res["tail"])
    digests = [json.loads((tmp_path / f"rank{r}.json").read_text()) for r in range(world)]
    assert digests[1] == digests[0], "rank 1 ended with different bytes than rank 0"
    assert digests[0]["report"] == ["GPU Culling", "Build HZB", "Lighting", "Sky", "Post Record", "TemporalAA", "AutoExposure", "Tonemap", "CAS"]
    assert digests[0]["next"][:3] == [0, 1, 1]  # after three frames of a ring of three: reads slot 0, writes slot 1, with history
    got = np.load(tmp_path / "rank0.npz")
    want = run_single(hotpath, 1920, 1080)
    for k, ((spec, _), (ldr, ring, lum)) in enumerate(zip(SEQUENCE, want)):
        assert np.array_equal(got[f"ldr{k}"], ldr.cpu().numpy()), (k, spec)
        for s, img in enumerate(ring):
            assert np.array_equal(got[f"ring{k}_{s}"], img.cpu().numpy()), (k, spec, s)
        both = np.concatenate([lum[0].cpu().numpy(), lum[1].cpu().numpy()])
        assert got[f"lum{k}"].view(np.uint32).tolist() == both.view(np.uint32).tolist(), (k, spec)
