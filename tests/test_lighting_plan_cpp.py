"""The host decisions of a Lighting launch (csrc/lighting_plan.cpp: the streaming launch's schedule, the staged cube's layout) without
a GPU: tests/cpp/test_lighting_plan.cpp, built by g++ from that one source. tests/golden/lighting_schedules.json holds what
ur_debug_lighting_schedule reported for launches on an MI355X before the planner was split out of the launch: the device's CU count,
the inputs, the eight words. The planner reproduces every row exactly."""
import json
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HERE = ROOT / "tests" / "cpp"
INPUTS = ("cus", "leave_cus", "ride_walkers", "balance", "pool_16ths", "chunk_shift", "stall", "w", "rows", "wpb", "tail_pending", "wide_pending", "grid_x", "grid_y")


def _build() -> Path:
    out = HERE / "_build"
    out.mkdir(exist_ok=True)
    exe = out / "test_lighting_plan"
    csrc = ROOT / "unclerenderer_amd" / "csrc"
    deps = [HERE / "test_lighting_plan.cpp", HERE / "lighting_plan_sweep.h", csrc / "lighting_plan.cpp", csrc / "lighting_plan.h"]
    if not exe.exists() or exe.stat().st_mtime <= max(d.stat().st_mtime for d in deps):
        cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", str(deps[0]), str(deps[2]), "-o", str(exe)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, f"{' '.join(cmd)}\n{r.stderr}"
    return exe


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_lighting_plan_cpp(tmp_path):
    rows = json.loads((ROOT / "tests" / "golden" / "lighting_schedules.json").read_text())
    assert len(rows) >= 25 and all(len(r["schedule"]) == 8 for r in rows)
    table = tmp_path / "schedules.txt"
    # claim words: the context owns kClaimWords = 32 of them (csrc/ur_internal.h)
    table.write_text("".join(" ".join(str(int(v)) for v in [r[k] for k in INPUTS] + [32 if r["claim_words"] else 0] + r["schedule"]) + "\n" for r in rows))
    r = subprocess.run([str(_build()), str(table)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and f"OK lighting plan: {len(rows)} recorded launches" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]


def test_env_cube_texels_is_the_layout_total(urlib):
    """ur_env_cube_texels needs no device: the library's entry point gives the sizes it gave before the layout was stated once."""
    want = {(256, 9): 1337154, (1, 1): 108, (2, 2): 312, (3, 2): 438, (256, 16): 1337910, (4096, 13): 335962602, (0, 3): 0, (8, 0): 0, (8, 17): 0}
    for (base, mips), texels in want.items():
        assert int(urlib.ur_env_cube_texels(base, mips)) == texels, (base, mips)
