"""The frame units (csrc/frame/*.cpp on csrc/rg/RenderGraph.cpp) without a GPU: tests/cpp/frame_trace.cpp, built by g++ from the tree's
frame sources, with a recording stand-in for every entry point they link against (the C ABI of the kernels, the check_* functions, the HIP
runtime). What the frame asks of them is compared with what the commit before the frame unit was split and planned asked:

tests/golden/frame_traces.txt holds, first, the curated cases (every pass, the five Tonemap launches and both CAS launches, the exchange with
and without TAA_BAND at world sizes 1, 2 and 4, rings of one and three images, a skipped finish_post, a failed pass in each half, setters
cleared between frames, both ride flags, the timing flags, every refusal in order): per case an FNV-1a digest of its full trace, and one
readable line per call with the entry points reached in order, the result, the report, hzb_ready and taa_next. Behind them one digest per
cell of two sweeps: every combination of the 18 scene-side flags with the post chain off (two frames each, 1024 cases per cell), and every
combination of the nine post flags over world size {1, 4}, ring {1, 3} and four frames (16 cases per cell).

It was recorded from that commit's csrc/frame/HotPathRenderer.cpp, byte for byte, compiled host-only with build.py's flags and linked with
these stand-ins (from the repository root, with that commit's tree in $PARENT):

    hipcc -O3 --offload-arch=gfx950 -fPIC -std=c++17 -fno-gpu-rdc -Wall -Wno-unused-function -Iinclude -x hip --offload-host-only \
        -c $PARENT/unclerenderer_amd/csrc/frame/HotPathRenderer.cpp -o HotPathRenderer.parent.o
    hipcc -O3 --offload-arch=gfx950 -fPIC -std=c++17 -fno-gpu-rdc -Iinclude -x hip --offload-host-only \
        -c $PARENT/unclerenderer_amd/csrc/rg/RenderGraph.cpp -o RenderGraph.parent.o
    g++ -std=c++17 -O1 -g -Wall -Iinclude -c tests/cpp/frame_trace.cpp -o frame_trace.o
    g++ frame_trace.o HotPathRenderer.parent.o RenderGraph.parent.o -o frame_trace_parent -pthread
    ./frame_trace_parent --record > tests/golden/frame_traces.txt

On a mismatch the program names the first differing case or cell and prints its trace in full; `frame_trace --case NAME` prints any case."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HERE = ROOT / "tests" / "cpp"
CSRC = ROOT / "unclerenderer_amd" / "csrc"
HIP_INCLUDE = Path("/opt/rocm/include")
FRAME_SOURCES = [CSRC / "frame" / n for n in ("FramePlan.cpp", "HotPathRenderer.cpp", "PostPasses.cpp", "LightingTimer.cpp", "FrameApi.cpp")] + [CSRC / "rg" / "RenderGraph.cpp"]
# (the HIP headers for the types alone: nothing of the runtime is linked)
HIP_FLAGS = ["-D__HIP_PLATFORM_AMD__", f"-I{HIP_INCLUDE}"]


def _build() -> Path:
    out = HERE / "_build"
    out.mkdir(exist_ok=True)
    exe = out / "frame_trace"
    sources = [HERE / "frame_trace.cpp"] + FRAME_SOURCES
    deps = sources + list((ROOT / "include").glob("*.h")) + list(CSRC.rglob("*.h"))
    if not exe.exists() or exe.stat().st_mtime <= max(d.stat().st_mtime for d in deps):
        cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", f"-I{ROOT / 'include'}"] + HIP_FLAGS + [str(s) for s in sources] + ["-o", str(exe), "-pthread"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, f"{' '.join(cmd)}\n{r.stderr}"
    return exe


@pytest.mark.skipif(shutil.which("g++") is None or not (HIP_INCLUDE / "hip" / "hip_runtime.h").exists(), reason="needs g++ and the HIP headers")
def test_frame_trace_cpp():
    r = subprocess.run([str(_build()), "--check", str(ROOT / "tests" / "golden" / "frame_traces.txt")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK frame trace: 54 curated cases, 262144 scene and 2048 post cases" in r.stdout, r.stdout[-8000:] + r.stderr[-2000:]


def test_frame_units_see_no_device_code():
    """The frame units include the host-only view of the internals (csrc/ur_checks.h), never ur_internal.h: that is what lets g++ build them."""
    for src in list((CSRC / "frame").glob("*")) + [CSRC / "ur_checks.h"]:
        assert "ur_internal.h\"" not in src.read_text(), src
