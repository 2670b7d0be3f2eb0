"""bench.py --dump-outputs end to end: two runs with the same arguments write the last timed frame's outputs as float32 /
float64 .npy files, within 64 MB, byte for byte the same. A plain run (no --full) runs no leg of its own behind the timed region.
The bench processes are children of the session's spawning helper (tests/_spawner.py), not of this process."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
STEPS = 6
ARGS = ["--gpus", "1", "--steps", str(STEPS), "--warmup", "2", "--min-warmup", "0"]


def _run(spawn_ranks, *extra: str) -> dict:
    res = spawn_ranks([sys.executable, str(ROOT / "bench.py"), *ARGS, *extra], [{}], timeout=300)
    tail = res["tail"][0]
    assert res["rc"] == [0], tail
    return json.loads(tail[tail.rindex('{"metric"'):].splitlines()[0])


def _bench(spawn_ranks, out: Path) -> dict:
    return _run(spawn_ranks, "--dump-outputs", str(out))


def test_dump_outputs_of_two_runs_are_the_same_bytes(hotpath, spawn_ranks, tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    ra = _bench(spawn_ranks, a)
    _bench(spawn_ranks, b)
    assert ra["steps"] == STEPS and ra["ms_per_step"] > 0
    names = sorted(p.name for p in a.glob("*.npy"))
    assert names == sorted(f"{n}.npy" for n in ra["dumped_outputs"])
    assert {"hdr.npy", "frame_rows.npy", "hzb.npy", "indirect_args.npy", "visible_indices.npy", "visible_count.npy"} <= set(names)
    assert sum((a / n).stat().st_size for n in names) <= 64 << 20
    for n in names:
        x, y = np.load(a / n), np.load(b / n)
        assert x.dtype in (np.float32, np.float64), n
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)), f"{n} differs between runs"
    hdr, rows = np.load(a / "hdr.npy"), np.load(a / "frame_rows.npy")
    assert hdr.shape == (rows.size, 3840, 4) and np.isfinite(hdr).all() and (hdr != 0).any()
    count = int(np.load(a / "visible_count.npy")[0])
    assert 0 < count <= 25 and np.load(a / "visible_indices.npy").shape == (count,)
    assert np.load(a / "indirect_args.npy").shape == (25, 16)


def test_a_plain_run_has_no_leg_of_its_own(hotpath, spawn_ranks):
    r = _run(spawn_ranks)
    assert r["steps"] == STEPS and r["value"] > 0 and r["ms_per_step"] > 0 and r["unit"] == "Mpixels/s"
    ro = r["roofline"]
    assert ro["launches_sampled"] > 0 and ro["frac"] > 0  # from the timed region's own samples
    assert not {"extras", "cpu_baseline", "with_python_gc_on", "dumped_outputs"} & set(r)
    assert not {"stream_ceiling", "other_inputs"} & set(ro)
    for k in ("alone_on_stream_us", "event_bracket_us", "event_record_us", "stream_ceiling_GBps", "traffic", "schedule"):
        assert ro[k] is None, k
