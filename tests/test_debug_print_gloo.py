"""dist.allreduce_cull_stats on CPU over gloo: the ranks' cull counters summed in place, on every rank (UR_FRAME_DEBUG_PRINT on row
bands prints the frame's totals)."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from unclerenderer_amd import dist as urdist


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        stats = torch.tensor([100 * rank + 7, 3 * rank], dtype=torch.int32)
        assert urdist.allreduce_cull_stats(stats) is None
        want = [sum(100 * r + 7 for r in range(world)), sum(3 * r for r in range(world))]
        assert stats.tolist() == want, (rank, stats.tolist(), want)
        again = torch.tensor([rank, 1], dtype=torch.int32)
        work = urdist.allreduce_cull_stats(again, async_op=True)
        work.wait()
        assert again.tolist() == [world * (world - 1) // 2, world]
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_allreduce_cull_stats(world):
    mp.spawn(_worker, args=(world, _free_port()), nprocs=world, join=True)


def test_single_rank_is_a_no_op():
    stats = torch.tensor([5, 6], dtype=torch.int32)
    assert urdist.allreduce_cull_stats(stats) is None and stats.tolist() == [5, 6]
