"""The post exchange across real rank processes: two and three FRESH processes (children of tests/_spawner.py; all on GPU 0 with
gloo, as tests/test_gpu_multirank.py does) each render their row band of the 1920x1080 C4 frame with UR_FRAME_POST_EXCHANGE, all-gather
the post records (dist.allgather_post_records, ring and direct in turn), run Frame.finish_post and all-gather the RGBA8 bands
(dist.allgather_rows). Over tests/_post_band_worker.SEQUENCE - with and without history, fused and not, a frame without
AutoExposure - every rank must end with the single-rank frame's image and EV, byte for byte."""
import json
import socket
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
WORKER = str(ROOT / "tests" / "_post_band_worker.py")


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("world", [2, 3])
def test_ranks_reproduce_the_single_rank_post_chain(hotpath, spawn_ranks, tmp_path, world):
    from tests._post_band_worker import SEQUENCE, run_single
    port = _port()
    envs = [dict(RANK=r, LOCAL_RANK=r, WORLD_SIZE=world, MASTER_ADDR="127.0.0.1", MASTER_PORT=port, HSA_ENABLE_IPC_MODE_LEGACY=0, OMP_NUM_THREADS=4)
            for r in range(world)]
    res = spawn_ranks([sys.executable, WORKER, "--out", str(tmp_path)], envs, timeout=540)
    assert res["rc"] == [0] * world, "rank processes failed:\n" + "\n----\n".join(res["tail"])
    digests = [json.loads((tmp_path / f"rank{r}.json").read_text()) for r in range(world)]
    for r in range(1, world):
        assert digests[r] == digests[0], f"rank {r} ended with different bytes than rank 0"
    report = digests[0]["report"]
    assert report == ["GPU Culling", "Build HZB", "Lighting", "Sky", "Post Record", "AutoExposure", "Tonemap", "CAS"], report
    got = np.load(tmp_path / "rank0.npz")
    want = run_single(hotpath, 1920, 1080)
    for k, ((spec, _, _), (ldr, lum)) in enumerate(zip(SEQUENCE, want)):
        assert np.array_equal(got[f"ldr{k}"], ldr.cpu().numpy()), (k, spec)
        if lum is not None:
            assert got[f"lum{k}"].view(np.uint32)[0] == lum.cpu().numpy().view(np.uint32)[0], (k, spec)
