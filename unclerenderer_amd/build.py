"""Build the in-tree native libraries with hipcc for gfx950 (no cmake, no JIT cache).

    python -m unclerenderer_amd.build [--force]

Outputs (git-ignored, shipped to the GPU box by gpurun):
    unclerenderer_amd/csrc/_build/libur_hotpath.so   HIP kernels + C-ABI (include/ur_hotpath.h, include/ur_host.h)
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "unclerenderer_amd" / "csrc"
OUT = CSRC / "_build"
LIB = OUT / "libur_hotpath.so"

ARCH = "gfx950"
COMMON = ["-O3", f"--offload-arch={ARCH}", "-fPIC", "-std=c++17", "-fno-gpu-rdc", "-Wall", "-Wno-unused-function",
          f"-I{ROOT / 'include'}"]
# exact-arithmetic translation units: no FMA contraction, IEEE divide (hipcc's default)
EXACT = ["-ffp-contract=off"]

# packed fp32 VALU ops are not faster on gfx950 and cost v_mov traffic; the atomic optimizer would turn the one-lane LDS
# work-counter claim into a scan + broadcast with an immediate wait
LIGHTING = ["-fno-slp-vectorize", "-mllvm", "-amdgpu-atomic-optimizer-strategy=None"]

# (source relative to csrc, extra flags)
SOURCES = [
    ("ur_api.hip", []),
    ("cull_api.hip", []),
    ("gather.hip", []),
    ("env_cube_stage.cpp", ["-x", "hip"]),  # (ur_api.hip's flags, which it was built with as a part of that unit)
    ("hzb.hip", EXACT),
    ("hzb_plan.cpp", ["-x", "hip"] + EXACT),
    ("cull.hip", EXACT),
    ("cull_views.hip", EXACT),
    ("cull_plan.cpp", ["-x", "hip"] + EXACT),
    ("lighting.hip", LIGHTING),
    ("lighting_tiled.hip", LIGHTING),
    ("lighting_host.hip", LIGHTING),  # host code only; the kernels' bits depend on its arithmetic, so it keeps their flags
    ("tonemap.hip", EXACT),
    ("taa.hip", EXACT),
    ("post.hip", EXACT),
    ("debug_print.hip", EXACT),
    ("raster.hip", EXACT),
    ("raster_mask.hip", EXACT),
    ("raster_pick.hip", EXACT),
    ("gbuffer_resolve.hip", EXACT),
    ("gbuffer_api.hip", EXACT),  # host code only: the entry points of the GBuffer and the Forward pass
    ("object_id_api.hip", EXACT),  # host code only: the entry points of the ObjectId pass and the pick
    ("forward_resolve.hip", EXACT),
    ("texture_transcode.hip", []),  # integer arithmetic alone: no flag changes its results
    ("mesh_build.hip", EXACT),
    ("scene_build.hip", EXACT),
    ("env_cube_build.hip", []),  # integer arithmetic alone: no flag changes its results
    ("env_prefilter.hip", EXACT),
    ("env_panorama.hip", EXACT),
    ("env_sky.hip", EXACT),
    ("brdf_lut.hip", EXACT),
    ("stream_ceiling.hip", []),
    ("scene.cpp", ["-x", "hip"] + EXACT),
    ("dds.cpp", ["-x", "hip"] + EXACT),
    ("hdr.cpp", ["-x", "hip"]),  # host code only, bytes alone: no flag changes its results
    ("host_math.cpp", ["-x", "hip"] + EXACT),
    ("bc_host.cpp", ["-x", "hip"]),  # host code only, over csrc/bc_decode.h: integer arithmetic, so no flag changes its results
    ("mesh_host.cpp", ["-x", "hip"] + EXACT),  # host code only, over csrc/mesh_rule.h: the rule the kernels of mesh_build.hip run
    ("scene_host.cpp", ["-x", "hip"] + EXACT),  # host code only, over csrc/scene_rule.h: the rule the kernels of scene_build.hip run
    ("env_cube_host.cpp", ["-x", "hip"]),  # host code only, over csrc/bc6h_decode.h: the decoder the kernels of env_cube_build.hip run
    ("env_prefilter_host.cpp", ["-x", "hip"] + EXACT),  # host code only, over csrc/env_prefilter_rule.h: the rule the kernels of env_prefilter.hip run
    ("env_panorama_host.cpp", ["-x", "hip"] + EXACT),  # host code only, over csrc/env_panorama_rule.h: the rule the kernel of env_panorama.hip runs
    ("env_sky_host.cpp", ["-x", "hip"] + EXACT),  # host code only, over csrc/env_sky_rule.h: the rule the kernel of env_sky.hip runs
    ("brdf_lut_host.cpp", ["-x", "hip"] + EXACT),  # host code only, over csrc/brdf_lut_rule.h: the rule the kernel of brdf_lut.hip runs
    ("lighting_plan.cpp", ["-x", "hip"] + EXACT),
    ("debug_font.cpp", ["-x", "hip"] + EXACT),
    ("rg/RenderGraph.cpp", ["-x", "hip"]),
    ("frame/FramePlan.cpp", ["-x", "hip"]),
    ("frame/HotPathRenderer.cpp", ["-x", "hip"]),
    ("frame/PostPasses.cpp", ["-x", "hip"]),
    ("frame/LightingTimer.cpp", ["-x", "hip"]),
    ("frame/FrameApi.cpp", ["-x", "hip"]),
]


def hipcc() -> str:
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not Path(exe).exists():
        raise RuntimeError("hipcc not found: the HIP extension cannot be built")
    return exe


def _deps() -> list[Path]:
    hdrs = list((ROOT / "include").glob("*.h")) + list(CSRC.rglob("*.h"))
    return hdrs


def _stale(target: Path, srcs: list[Path]) -> bool:
    if not target.exists():
        return True
    t = target.stat().st_mtime
    return any(s.stat().st_mtime > t for s in srcs if s.exists())


def _compile(job) -> Path:
    src, flags, force = job
    srcp = CSRC / src
    obj = OUT / (src.replace("/", "_") + ".o")
    if force or _stale(obj, [srcp] + _deps()):
        cmd = [hipcc()] + COMMON + flags + ["-c", str(srcp), "-o", str(obj)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed for {src}:\n{' '.join(cmd)}\n{r.stdout}\n{r.stderr}")
        if r.stderr.strip():
            sys.stderr.write(r.stderr)
    return obj


def build(force: bool = False, verbose: bool = False) -> Path:
    OUT.mkdir(parents=True, exist_ok=True)
    present = [(s, f, force) for s, f in SOURCES if (CSRC / s).exists()]
    with ThreadPoolExecutor(max_workers=min(4, os.cpu_count() or 1)) as ex:
        objs = list(ex.map(_compile, present))
    if force or _stale(LIB, objs):
        cmd = [hipcc(), f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", str(LIB)] + [str(o) for o in objs] + ["-ldl", "-lpthread"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"link failed:\n{' '.join(cmd)}\n{r.stdout}\n{r.stderr}")
    if verbose:
        print(f"built {LIB}")
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv, verbose=True)
