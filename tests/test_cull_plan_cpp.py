"""The host decisions of CullIndirectArgs (csrc/cull_plan.cpp: the launches of one call, the workspace and its slices, flavour 4's record,
the dispatch that carries ur_time_next_cull's event) without a GPU: tests/cpp/test_cull_plan.cpp, built by g++ from that one source.
tests/golden/cull_plans.txt holds what cull_launches did for a sweep of calls before the planner was split out of it (its launches and
its ur_reserve replaced by prints). The planner reproduces every row exactly."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HERE = ROOT / "tests" / "cpp"


def _build() -> Path:
    out = HERE / "_build"
    out.mkdir(exist_ok=True)
    exe = out / "test_cull_plan"
    csrc = ROOT / "unclerenderer_amd" / "csrc"
    deps = [HERE / "test_cull_plan.cpp", HERE / "cull_plan_sweep.h", csrc / "cull_plan.cpp", csrc / "cull_plan.h", ROOT / "include" / "ur_hotpath.h"]
    if not exe.exists() or exe.stat().st_mtime <= max(d.stat().st_mtime for d in deps):
        cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", str(deps[0]), str(deps[2]), "-o", str(exe)]  # (no HIP include path: plain C++)
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, f"{' '.join(cmd)}\n{r.stderr}"
    return exe


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_cull_plan_cpp():
    golden = ROOT / "tests" / "golden" / "cull_plans.txt"
    rows = [line for line in golden.read_text().splitlines() if line and not line.startswith("#")]
    assert len(rows) <= 2000
    did = [r.split(" | ")[1] for r in rows]
    # the table covers what it has to: every kind, both RANGES choices, a reserve, a valid record, every launch that can carry the event,
    # every sweep value of n
    for kind in ("nothing ", "zero ", "single ", "multi "):
        assert any(d.startswith(kind) for d in did), kind
    for kind in ("single", "multi"):
        for ranges in (0, 1):
            assert any(d.startswith(f"{kind} ranges {ranges} ") for d in did), (kind, ranges)
    assert any(" reserve 0 " not in d for d in did if d.startswith("multi"))
    assert any(" valid 1 " in d for d in did)
    for stop in ("only", "cull", "compaction", "none"):
        assert any(f" stop {stop} " in d for d in did), stop
    for n in (0, 1, 255, 256, 257, 512, 513, 16384, 16385, 70_000, 1_000_000):
        assert any(r.startswith(f"n {n} ") for r in rows), n
    assert "n 257 list 0 ranges 0 views 4 compacted 15 most 260 flavour 3 record 0 1 ws 512 stop 0 | multi ranges 0 blocks 2 compact 1 grid 1 5 workspace 1 reserve 0 ws 512 stride 2 slices 1 2 3 4 valid 0 keep 0 stop none carried 0" in rows
    r = subprocess.run([str(_build()), str(golden)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and f"OK cull plan: {len(rows)} recorded calls" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
