"""The host decisions of Build HZB (csrc/hzb_plan.cpp: the chain's steps, its layout, a band's share) without a GPU:
tests/cpp/test_hzb_plan.cpp, built by g++ from that one source. tests/golden/hzb_chains.txt holds the steps the launch loop of
csrc/hzb.hip took, for ur_build_hzb, ur_build_hzb_band and ur_build_hzb_tail under every ur_defer_hzb_tail mode, before the planner
was split out of it (its launches and holds replaced by prints). The planner reproduces every row exactly."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HERE = ROOT / "tests" / "cpp"
SIZES = [(1, 1), (2, 2), (3, 5), (17, 9), (64, 64), (129, 67), (512, 512), (1000, 3), (5, 300), (2, 33), (4096, 16), (1920, 1080), (3840, 2160),
         (6001, 3999), (7680, 4320), (16384, 4200), (65536, 1100)]


def _build() -> Path:
    out = HERE / "_build"
    out.mkdir(exist_ok=True)
    exe = out / "test_hzb_plan"
    csrc = ROOT / "unclerenderer_amd" / "csrc"
    deps = [HERE / "test_hzb_plan.cpp", HERE / "hzb_plan_sweep.h", csrc / "hzb_plan.cpp", csrc / "hzb_plan.h", ROOT / "include" / "ur_hotpath.h"]
    if not exe.exists() or exe.stat().st_mtime <= max(d.stat().st_mtime for d in deps):
        cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", str(deps[0]), str(deps[2]), "-o", str(exe)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, f"{' '.join(cmd)}\n{r.stderr}"
    return exe


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_hzb_plan_cpp():
    golden = ROOT / "tests" / "golden" / "hzb_chains.txt"
    rows = [line for line in golden.read_text().splitlines() if line and not line.startswith("#")]
    # the table covers what it has to: every size under modes 0, 1, 2, 2160 rows over 1, 2, 4, 8 ranks, a chain the band form refuses
    for w, h in SIZES:
        for mode in (0, 1, 2):
            assert any(r.startswith(f"chain {w} {h} mode {mode} done 1 |") for r in rows), (w, h, mode)
    assert sum(r.startswith("band 3840 2160 mode 2 pieces") and r.endswith("hold") for r in rows) == 1 + 2 + 4 + 8
    assert any(r.startswith("band ") and r.endswith("| refused") for r in rows)
    assert "chain 16384 4200 mode 0 done 1 | wide 0 4 depth 128 132 0 launch | wide 4 4 mip 8 9 0 launch | tail 8 6 launch" in rows
    r = subprocess.run([str(_build()), str(golden)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and f"OK hzb plan: {len(rows)} recorded chains" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
