"""The post exchange of row bands (UR_FRAME_POST_EXCHANGE) without a GPU: the flag, the new symbols and their argument checks, the
record size, the gfx950 code of the new kernels, a numpy model of which rank owns each AutoExposure tap texel, and
dist.allgather_post_records over gloo."""
import ctypes as C
import os
import re
import socket
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.code_objects import LLVM, library_kernels

ROOT = Path(__file__).resolve().parent.parent
F = np.float32
NEW = ("ur_post_record_bytes", "ur_pack_post_record", "ur_auto_exposure_records", "ur_tonemap_cas_halo", "ur_cas_halo",
       "ur_frame_set_post_records", "ur_frame_finish_post")

# the sizes tests/test_gpu_post_band.py splits into virtual bands: (w, h, [N...])
GPU_SIZES = [(1, 1, [1]), (7, 5, [1]), (64, 24, [3]), (48, 48, [3]), (40, 8, [8]), (16, 16, [8, 16]), (1920, 1080, [2, 4, 8]),
             (3840, 2160, [2, 3, 8]), (7680, 4320, [8])]


def test_flag_does_not_collide():
    from unclerenderer_amd import lib
    assert lib.UR_FRAME_POST_EXCHANGE == 0x200000
    others = [getattr(lib, n) for n in dir(lib) if n.startswith("UR_FRAME_") and n not in ("UR_FRAME_POST_EXCHANGE", "UR_FRAME_DEFAULT")]
    assert len(others) >= 20 and all(o & lib.UR_FRAME_POST_EXCHANGE == 0 for o in others)
    header = (ROOT / "include" / "ur_frame.h").read_text()
    defined = {m.group(1): int(m.group(2), 16) for m in re.finditer(r"#define (UR_FRAME_\w+) 0x([0-9a-fA-F]+)u", header)}
    assert defined["UR_FRAME_POST_EXCHANGE"] == 0x200000 and len(set(defined.values())) == len(defined)


def test_symbols_declared_exported_and_bound(urlib):
    from unclerenderer_amd import lib
    text = "".join(re.sub(r"/\*.*?\*/", "", (ROOT / "include" / h).read_text(), flags=re.S) for h in ("ur_hotpath.h", "ur_frame.h"))
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in lib.SIGNATURES and getattr(urlib, name) is not None
    if not (LLVM / "llvm-readelf").exists():
        pytest.skip("llvm tools not found")
    dyn = subprocess.run([str(LLVM / "llvm-readelf"), "--dyn-syms", "--wide", str(lib.library_path())], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert re.search(r"FUNC\s+GLOBAL\s+DEFAULT\s+\d+\s+%s$" % name, dyn, re.M), name


def test_record_bytes(urlib):
    from unclerenderer_amd.hotpath import post_record_bytes
    for w in (1, 7, 16, 1920, 3840, 7680):
        assert urlib.ur_post_record_bytes(w) == post_record_bytes(w) == (2 * w + 1024) * 8
    assert post_record_bytes(3840) == 69632  # about 70 KB per rank at 4K
    assert urlib.ur_post_record_bytes(0xFFFFFFFF) == (2 * 0xFFFFFFFF + 1024) * 8  # no 32-bit wrap


def test_null_and_bad_arguments_are_rejected(urlib):
    from unclerenderer_amd import lib
    ae = lib.AutoExposureConstants((C.c_float * 2)(16, 16), 0.0, 3.0, 1.0, 0, 0.3, 0.1, 5.0)
    cas = lib.CasConstants((C.c_float * 2)(1 / 16, 1 / 16), 0.5, 0.0)
    tm = lib.TonemapConstants(1, 0, 0.9, 2.2)
    buf = (C.c_uint64 * 8192)()
    base = C.addressof(buf)
    p, q, r = C.c_void_p(base), C.c_void_p(base + 16384), C.c_void_p(base + 32768)
    E = lib.UR_EINVAL
    # null context / pointers
    assert urlib.ur_pack_post_record(None, p, 16, 16, 0, 16, q) == E
    assert urlib.ur_auto_exposure_records(None, C.byref(ae), p, 1, 16, 16, None, q) == E
    assert urlib.ur_tonemap_cas_halo(None, C.byref(tm), C.byref(cas), p, None, None, None, q, 16, 16, 0, 16) == E
    assert urlib.ur_cas_halo(None, C.byref(tm), C.byref(cas), p, None, None, None, q, 16, 16, 0, 16) == E
    assert urlib.ur_frame_set_post_records(None, p, q) == E
    assert urlib.ur_frame_finish_post(None) == E
    assert "null" in urlib.ur_last_error().decode()
    # bad arguments are rejected before anything touches the context (a stand-in that is never dereferenced)
    ctx = C.c_void_p(base + 60000)
    assert urlib.ur_pack_post_record(ctx, p, 16, 16, 8, 9, q) == E           # out of the frame
    assert urlib.ur_pack_post_record(ctx, p, 16, 16, 0, 0, q) == E           # empty
    assert urlib.ur_pack_post_record(ctx, p, 16, 16, 0, 16, C.c_void_p(base + 8)) == E  # the record overlaps the band
    assert urlib.ur_auto_exposure_records(ctx, C.byref(ae), p, 3, 16, 16, None, q) == E   # 3 does not divide 16
    assert urlib.ur_auto_exposure_records(ctx, C.byref(ae), p, 0, 16, 16, None, q) == E
    assert urlib.ur_auto_exposure_records(ctx, C.byref(ae), p, 2, 16, 8, None, q) == E    # InputSize != (w, h)
    ae_hist = lib.AutoExposureConstants((C.c_float * 2)(16, 16), 0.0, 3.0, 1.0, 1, 0.3, 0.1, 5.0)
    assert urlib.ur_auto_exposure_records(ctx, C.byref(ae_hist), p, 2, 16, 16, None, q) == E  # history without prev_ev
    for fn in (urlib.ur_tonemap_cas_halo, urlib.ur_cas_halo):
        assert fn(ctx, C.byref(tm), C.byref(cas), p, None, r, None, q, 16, 16, 4, 4) == E   # row0 > 0 needs hdr_above
        assert "hdr_above" in urlib.ur_last_error().decode()
        assert fn(ctx, C.byref(tm), C.byref(cas), p, r, None, None, q, 16, 16, 4, 4) == E   # row0 + rows < h needs hdr_below
        assert fn(ctx, C.byref(tm), C.byref(cas), p, None, None, None, q, 16, 16, 0, 17) == E  # out of the frame
        assert fn(ctx, C.byref(tm), C.byref(cas), p, r, r, None, C.c_void_p(base + 32768 - 64), 16, 16, 4, 4) == E  # out overlaps a halo row
        assert fn(ctx, C.byref(tm), C.byref(cas), p, None, None, None, C.c_void_p(base + 64), 16, 16, 0, 16) == E  # out overlaps the band
        bad = lib.CasConstants((C.c_float * 2)(1 / 8, 1 / 16), 0.5, 0.0)
        assert fn(ctx, C.byref(tm), C.byref(bad), p, None, None, None, q, 16, 16, 0, 16) == lib.UR_EUNSUPPORTED


def test_new_kernels_use_no_scratch(urlib, tmp_path):
    """post_record_kernel, ae_records_kernel and the four cas_halo_kernel forms: no scratch, no spills; and the names the existing
    count of cas_strip_kernel / auto_exposure_kernel forms relies on are not reused."""
    if not (LLVM / "llvm-readelf").exists():
        pytest.skip("llvm tools not found")
    meta = library_kernels(tmp_path)
    new = {k: v for k, v in meta.items() if any(n in k for n in ("post_record_kernel", "ae_records_kernel", "cas_halo_kernel"))}
    assert len(new) == 6, sorted(new)
    assert sum("cas_halo_kernel" in k for k in new) == 4
    for name, m in new.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
    assert len([k for k in meta if "cas_strip_kernel" in k or "auto_exposure_kernel" in k]) == 5


# ---- the ownership of the tap texels ---------------------------------------------------------------------------------------

def ae_taps(w: int, h: int):
    """(x0, x1, y0, y1, ax, ay) of the 256 taps in tap order, as ae_tap computes them (fp32, no contraction, IEEE divide)."""
    g = np.arange(256)
    gx, gy = (g & 15).astype(F), (g >> 4).astype(F)
    sx, sy = F(w), F(h)
    px, py = (gx + F(0.5)) * (sx / F(16)), (gy + F(0.5)) * (sy / F(16))
    u, v = px / np.maximum(sx, F(1)), py / np.maximum(sy, F(1))
    tx, ty = u * F(w) - F(0.5), v * F(h) - F(0.5)
    fx, fy = np.floor(tx), np.floor(ty)
    ix, iy = fx.astype(np.int64), fy.astype(np.int64)
    c = lambda a, m: np.clip(a, 0, m)
    return c(ix, w - 1), c(ix + 1, w - 1), c(iy, h - 1), c(iy + 1, h - 1), tx - fx, ty - fy


def slot_rows(w, h):
    """The row of each of the 1024 texel slots (tap i, corner t00, t10, t01, t11)."""
    _, _, y0, y1, _, _ = ae_taps(w, h)
    return np.stack([y0, y0, y1, y1], axis=1).reshape(-1)


def straddles(w, h, n):
    """Taps whose two rows belong to different bands: (with non-zero y weight, with y weight 0)."""
    _, _, y0, y1, _, ay = ae_taps(w, h)
    band = h // n
    s = (y0 // band) != (y1 // band)
    return int((s & (ay != 0)).sum()), int((s & (ay == 0)).sum())


@pytest.mark.parametrize("w,h", [(1, 1), (7, 5), (16, 16), (40, 8), (64, 24), (48, 48), (33, 45), (100, 18), (1904, 1052), (1920, 1080),
                                 (3840, 2160), (7680, 4320)])
def test_every_tap_slot_is_owned_exactly_once(w, h):
    rows = slot_rows(w, h)
    assert rows.min() >= 0 and rows.max() < h
    for n in [d for d in range(1, min(h, 16) + 1) if h % d == 0]:
        band = h // n
        owners = np.zeros(rows.size, np.int64)
        for r in range(n):  # what post_record_kernel writes: the texel where its row lies in the band
            owners += (rows >= r * band) & (rows < (r + 1) * band)
        assert (owners == 1).all(), (w, h, n)
        assert ((rows // band) < n).all()  # the owner ae_records_kernel reads


def test_the_gpu_sizes_include_straddling_taps():
    """The design must not rely on a tap's two rows lying in one band: the GPU sizes include taps across a band edge with non-zero
    weight (64x24 and 16x16 / 40x8 one-row bands) and with weight 0 (48x48 with N = 3: only 0 * Inf shows the far row)."""
    hits = {(w, h, n): straddles(w, h, n) for w, h, ns in GPU_SIZES for n in ns}
    assert hits[(64, 24, 3)] == (32, 0) and hits[(40, 8, 8)] == (224, 0)   # non-zero y weight across an edge
    assert hits[(48, 48, 3)] == (0, 16) and hits[(16, 16, 16)] == (0, 240)  # weight 0 across an edge
    assert hits[(3840, 2160, 8)] == (0, 0) and hits[(7680, 4320, 8)] == (0, 0)  # production sizes: none
    # the ranges the issue names: non-zero weight across an edge at H = 18..45 with N = 3 and at H = N < 16 (16: weight 0)
    assert all(straddles(64, h, 3)[0] > 0 for h in range(18, 46, 3))
    assert all(straddles(32, n, n)[0] > 0 for n in range(2, 16))


# ---- allgather_post_records over gloo -----------------------------------------------------------------------------------------

def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _record(rank, nbytes):
    return torch.from_numpy(np.random.default_rng(100 + rank).integers(0, 256, nbytes, dtype=np.uint8))


def _records_worker(rank, world, port, nbytes, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from unclerenderer_amd import dist as urdist
        want = torch.stack([_record(r, nbytes) for r in range(world)])
        for mode in ("ring", "direct"):
            # a record of its own
            allr = torch.zeros((world, nbytes), dtype=torch.uint8)
            assert urdist.allgather_post_records(allr, _record(rank, nbytes), mode=mode) is None
            assert torch.equal(allr, want), mode
            # in place: the record packed straight into its row of the gathered buffer; and the handle form
            allr = torch.zeros((world, nbytes), dtype=torch.uint8)
            allr[rank].copy_(_record(rank, nbytes))
            work = urdist.allgather_post_records(allr, allr[rank], async_op=True, mode=mode)
            work.wait()
            assert torch.equal(allr, want), mode
        np.save(os.path.join(out_dir, f"rec{rank}.npy"), allr.numpy())
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_allgather_post_records_over_gloo(tmp_path, world):
    from unclerenderer_amd.hotpath import post_record_bytes
    nbytes = post_record_bytes(40)
    mp.spawn(_records_worker, args=(world, _free_port(), nbytes, str(tmp_path)), nprocs=world, join=True)
    want = np.stack([_record(r, nbytes).numpy() for r in range(world)])
    for r in range(world):
        assert np.array_equal(np.load(tmp_path / f"rec{r}.npy"), want)


def test_allgather_post_records_one_rank():
    from unclerenderer_amd import dist as urdist
    allr = torch.zeros((1, 64), dtype=torch.uint8)
    assert urdist.allgather_post_records(allr, _record(0, 64)) is None
    assert torch.equal(allr[0], _record(0, 64))
