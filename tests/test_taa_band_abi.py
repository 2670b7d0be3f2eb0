"""TemporalAA on row bands (UR_FRAME_TAA_BAND) without a GPU: the flag, the new symbols and their argument checks, the TAA record's
size, the gfx950 code of the new kernels, and dist.allgather_taa_records over gloo."""
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

ROOT = Path(__file__).resolve().parent.parent
LLVM = Path("/opt/rocm/lib/llvm/bin")
NEW = ("ur_taa_record_bytes", "ur_pack_taa_record", "ur_temporal_aa_halo", "ur_temporal_aa_tonemap_halo", "ur_frame_set_taa_records")


def test_flag_value_and_distinctness():
    from unclerenderer_amd import lib
    assert lib.UR_FRAME_TAA_BAND == 0x2000000
    others = [getattr(lib, n) for n in dir(lib) if n.startswith("UR_FRAME_") and n not in ("UR_FRAME_TAA_BAND", "UR_FRAME_DEFAULT")]
    assert len(others) >= 24 and all(o & lib.UR_FRAME_TAA_BAND == 0 for o in others)
    assert lib.UR_FRAME_DEFAULT & lib.UR_FRAME_TAA_BAND == 0
    header = (ROOT / "include" / "ur_frame.h").read_text()
    defined = {m.group(1): int(m.group(2), 16) for m in re.finditer(r"#define (UR_FRAME_\w+) 0x([0-9a-fA-F]+)u", header)}
    assert defined["UR_FRAME_TAA_BAND"] == 0x2000000 and len(set(defined.values())) == len(defined)
    assert {k: v for k, v in defined.items()} == {k: getattr(lib, k) for k in defined}  # every flag of the header is bound with its value


def test_symbols_declared_exported_and_bound(urlib):
    from unclerenderer_amd import dist as urdist
    from unclerenderer_amd import lib
    from unclerenderer_amd.hotpath import Frame, HotPath
    text = "".join(re.sub(r"/\*.*?\*/", "", (ROOT / "include" / h).read_text(), flags=re.S) for h in ("ur_hotpath.h", "ur_frame.h"))
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in lib.SIGNATURES and getattr(urlib, name) is not None
    for cls, names in ((HotPath, ("temporal_aa_halo", "temporal_aa_tonemap_halo", "pack_taa_record", "taa_record_bytes")), (Frame, ("set_taa_records",)),
                       (urdist, ("allgather_taa_records",))):
        for n in names:
            assert callable(getattr(cls, n)), n
    if not (LLVM / "llvm-readelf").exists():
        pytest.skip("llvm tools not found")
    dyn = subprocess.run([str(LLVM / "llvm-readelf"), "--dyn-syms", "--wide", str(lib.library_path())], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert re.search(r"FUNC\s+GLOBAL\s+DEFAULT\s+\d+\s+%s$" % name, dyn, re.M), name


def test_record_bytes(urlib):
    from unclerenderer_amd.hotpath import post_record_bytes, taa_record_bytes
    for w in (1, 7, 16, 1920, 3840, 7680):
        assert urlib.ur_taa_record_bytes(w) == taa_record_bytes(w) == 32 * w
    assert urlib.ur_taa_record_bytes(0xFFFFFFFF) == 32 * 0xFFFFFFFF  # no 32-bit wrap
    # what a rank sends per frame at 4K: (2w + 1024) * 8 + 32w bytes, about 184 KB, against an 8.3 MB RGBA16F band of 8 ranks
    assert post_record_bytes(3840) + taa_record_bytes(3840) == (2 * 3840 + 1024) * 8 + 32 * 3840 == 192512
    assert 3840 * (2160 // 8) * 8 == 8294400


def _buffers():
    buf = (C.c_uint64 * 16384)()  # 128 KiB of host memory: stand-ins for device pointers that are never dereferenced
    base = C.addressof(buf)
    return buf, base, [C.c_void_p(base + k * 8192) for k in range(14)]


def test_pack_argument_checks(urlib):
    from unclerenderer_amd import lib
    buf, base, (p, q, r, *_) = _buffers()
    E, U = lib.UR_EINVAL, lib.UR_EUNSUPPORTED
    f = urlib.ur_pack_taa_record
    assert f(None, p, q, 1, 16, 16, 0, 8, r) == E and "null" in urlib.ur_last_error().decode()
    ctx = C.c_void_p(base + 120000)  # a stand-in: every check below returns before the context is used
    assert f(ctx, None, q, 1, 16, 16, 0, 8, r) == E      # no band
    assert f(ctx, p, None, 1, 16, 16, 0, 8, r) == E      # history wanted, none given
    assert f(ctx, p, q, 1, 16, 16, 0, 8, None) == E      # no record
    assert f(ctx, p, q, 1, 16, 16, 12, 8, r) == E        # out of the frame
    assert f(ctx, p, q, 1, 16, 16, 0, 0, r) == E         # empty
    assert f(ctx, p, q, 1, 0, 16, 0, 8, r) == E
    assert f(ctx, p, q, 1, 16, 16, 4, 1, r) == U         # a one-row band that is not the whole frame
    assert "2 rows" in urlib.ur_last_error().decode()
    assert f(ctx, p, q, 1, 16, 16, 0, 8, C.c_void_p(base + 64)) == E            # the record overlaps the band
    assert f(ctx, p, q, 1, 16, 16, 0, 8, C.c_void_p(base + 8192 + 64)) == E     # ... the history band
    assert "overlaps" in urlib.ur_last_error().decode()


def test_halo_argument_checks(urlib):
    """Null is allowed exactly where the band touches the frame's edge; the pointers of a resolved row come together."""
    from unclerenderer_amd import lib
    buf, base, (cur, ab, be, his, out, a2, ha, b2, hb, ra, rb, ldr, *_) = _buffers()
    tm = lib.TonemapConstants(1, 0, 0.9, 2.2)
    E = lib.UR_EINVAL
    ctx = C.c_void_p(base + 120000)
    N = None

    def plain(*a):
        return urlib.ur_temporal_aa_halo(*a)

    def fused(c, cur_, ab_, be_, his_, out_, *rest):
        return urlib.ur_temporal_aa_tonemap_halo(c, C.byref(tm), cur_, ab_, be_, his_, out_, None, ldr, *rest)

    for f in (plain, fused):
        tail = (0.9, 1, 16, 16, 4, 4)  # a band with a neighbour on both sides
        assert f(None, cur, ab, be, his, out, N, N, N, N, N, N, *tail) == E          # null context
        assert f(ctx, None, ab, be, his, out, N, N, N, N, N, N, *tail) == E          # no current band
        assert f(ctx, cur, ab, be, None, out, N, N, N, N, N, N, *tail) == E          # history wanted, none given
        assert f(ctx, cur, ab, be, his, None, N, N, N, N, N, N, *tail) == E          # no output
        assert f(ctx, cur, None, be, his, out, N, N, N, N, N, N, *tail) == E         # row0 > 0 needs cur_above
        assert "cur_above" in urlib.ur_last_error().decode()
        assert f(ctx, cur, ab, None, his, out, N, N, N, N, N, N, *tail) == E         # row0 + rows < h needs cur_below
        assert f(ctx, cur, ab, be, his, out, N, N, N, N, N, N, 0.9, 1, 16, 16, 14, 4) == E   # out of the frame
        assert f(ctx, cur, ab, be, his, out, N, N, N, N, N, N, 0.9, 1, 16, 16, 4, 0) == E    # empty band
        # at the frame's edges the side's pointers must be null
        assert f(ctx, cur, ab, be, his, out, N, N, N, N, N, N, 0.9, 1, 16, 16, 0, 4) == E    # cur_above at the top edge
        assert "edge" in urlib.ur_last_error().decode()
        assert f(ctx, cur, ab, be, his, out, N, N, N, N, N, N, 0.9, 1, 16, 16, 12, 4) == E   # cur_below at the bottom edge
        assert f(ctx, cur, N, be, his, out, a2, ha, N, N, ra, N, 0.9, 1, 16, 16, 0, 4) == E  # a resolved row above the frame
        assert f(ctx, cur, ab, N, his, out, N, N, b2, hb, N, rb, 0.9, 1, 16, 16, 12, 4) == E
        # a resolved row needs its second current row and, with history, the neighbour's history row; none without it
        assert f(ctx, cur, ab, be, his, out, N, ha, N, N, ra, N, *tail) == E     # resolved_above without above2
        assert "above2" in urlib.ur_last_error().decode()
        assert f(ctx, cur, ab, be, his, out, a2, N, N, N, ra, N, *tail) == E     # ... without hist_above while use_history
        assert f(ctx, cur, ab, be, his, out, a2, ha, N, N, N, N, *tail) == E     # above2 without resolved_above
        assert f(ctx, cur, ab, be, his, out, N, N, b2, N, N, rb, *tail) == E     # resolved_below without hist_below
        assert f(ctx, cur, ab, be, his, out, N, N, N, hb, N, N, *tail) == E      # hist_below alone
        # aliasing: a resolved row over an input, the output over the current band (history in place is allowed, and not tested here:
        # a valid call would launch)
        assert f(ctx, cur, ab, be, his, out, a2, ha, N, N, ab, N, *tail) == E
        assert f(ctx, cur, ab, be, his, out, a2, ha, b2, hb, ra, ra, *tail) == E
        assert "overlap" in urlib.ur_last_error().decode()
        assert f(ctx, cur, ab, be, his, cur, N, N, N, N, N, N, *tail) == E
    # the fused form's own arguments
    assert urlib.ur_temporal_aa_tonemap_halo(ctx, None, cur, ab, be, his, out, None, ldr, N, N, N, N, N, N, 0.9, 1, 16, 16, 4, 4) == E
    assert urlib.ur_temporal_aa_tonemap_halo(ctx, C.byref(tm), cur, ab, be, his, out, None, None, N, N, N, N, N, N, 0.9, 1, 16, 16, 4, 4) == E
    assert "ur_temporal_aa_tonemap_halo" in urlib.ur_last_error().decode()


def test_frame_argument_checks(urlib):
    """ur_frame_set_taa_records and render's UR_FRAME_TAA_BAND checks on frames over a stand-in context, in the style of
    tests/test_taa_abi.py::test_frame_ring_argument_checks: every check returns before the context or a device pointer is used."""
    from unclerenderer_amd import lib
    buf, base, ptrs = _buffers()
    ctx = C.c_void_p(base + 120000)
    E, U = lib.UR_EINVAL, lib.UR_EUNSUPPORTED
    assert urlib.ur_frame_set_taa_records(None, ptrs[0], ptrs[1]) == E
    TM, TAA, BAND, PX = lib.UR_FRAME_TONEMAP, lib.UR_FRAME_TAA, lib.UR_FRAME_TAA_BAND, lib.UR_FRAME_POST_EXCHANGE
    FT, FC, CAS = lib.UR_FRAME_FUSE_TAA_TONEMAP, lib.UR_FRAME_FUSE_TONEMAP_CAS, lib.UR_FRAME_CAS
    cc = (C.c_uint32 * lib.UR_CULL_CONSTANT_DWORDS)()
    scene, sky = lib.SceneConstants(), lib.SkyConstants()

    def ring(n):
        arr = (C.c_void_p * n)(*[base + 4096 * (k + 1) for k in range(n)])
        t = lib.FrameTaa(C.cast(arr, C.POINTER(C.c_void_p)), n, 0.9)
        t._keep = arr
        return t

    f = C.c_void_p(urlib.ur_frame_create(ctx, None, 3, 1, 2))  # rank 1 of 2
    assert f
    try:
        res = lib.FrameResources()
        res.width, res.height, res.row0, res.rows = 16, 16, 8, 8
        res.tonemap_band = base

        def render(flags):
            return urlib.ur_frame_render(f, C.byref(res), cc, C.byref(scene), C.byref(sky), flags)

        full = TM | TAA | BAND | PX
        assert urlib.ur_frame_set_taa_records(f, None, ptrs[1]) == E and urlib.ur_frame_set_taa_records(f, ptrs[0], None) == E
        assert render(full) == E and "ur_frame_set_taa" in urlib.ur_last_error().decode()       # no ring
        assert urlib.ur_frame_set_taa(f, C.byref(ring(3))) == lib.UR_OK
        assert render(full) == E and "ur_frame_set_post_records" in urlib.ur_last_error().decode()  # no post records
        assert urlib.ur_frame_set_post_records(f, ptrs[2], ptrs[3]) == lib.UR_OK
        assert render(full) == E and "ur_frame_set_taa_records" in urlib.ur_last_error().decode()   # no TAA records
        assert urlib.ur_frame_set_taa_records(f, ptrs[4], ptrs[5]) == lib.UR_OK
        # the flag without TAA / without the exchange; without it the two answers of before
        assert render(TM | BAND | PX) == E and "TAA_BAND needs" in urlib.ur_last_error().decode()
        assert render(TM | TAA | BAND) == E and "TAA_BAND needs" in urlib.ur_last_error().decode()
        assert render(BAND) == E
        assert render(TM | TAA | PX) == U and render(TM | TAA) == U
        assert "whole frame" in urlib.ur_last_error().decode()
        assert render(TAA | BAND | PX) == E                                                  # no TONEMAP
        assert render(full | FT | CAS | FC) == E and "exclude" in urlib.ur_last_error().decode()  # both fusions
        res.tonemap_band = None
        assert render(full) == E
        res.tonemap_band = base
        # not rank 1's equal band
        res.row0 = 0
        assert render(full) == E and "equal band" in urlib.ur_last_error().decode()
        res.row0, res.rows = 8, 4
        assert render(full) == E
        # one-row bands of several ranks
        res.height, res.row0, res.rows = 2, 1, 1
        assert render(full) == U and "2 rows" in urlib.ur_last_error().decode()
        assert urlib.ur_frame_finish_post(f) == E  # nothing was rendered: nothing is pending
    finally:
        urlib.ur_frame_destroy(f)


def test_new_kernels_use_no_scratch(urlib, tmp_path):
    """taa_band_kernel (plain and Tonemap forms) and taa_record_kernel: no scratch, no VGPR or SGPR spills, and within the register
    budget of the strip kernel they share their body with (8 waves per SIMD: at most 64 VGPRs). Their names contain none of the
    substrings by which the existing tests count kernels."""
    from tests.code_objects import code_objects, kernel_metadata
    from unclerenderer_amd import lib
    if not (LLVM / "llvm-readelf").exists():
        pytest.skip("llvm tools not found")
    meta = {}
    for co in code_objects(lib.library_path(), tmp_path):
        meta.update(kernel_metadata(co))
    new = {k: v for k, v in meta.items() if "taa_band_kernel" in k or "taa_record_kernel" in k}
    assert len(new) == 3, sorted(new)
    assert sum("taa_band_kernel" in k and "NoPost" in k for k in new) == 1 and sum("taa_band_kernel" in k and "TonemapPost" in k for k in new) == 1
    for name, m in new.items():
        print(name, m)
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
        assert m["vgpr_count"] <= 64, (name, m)
    for name in new:
        assert not any(s in name for s in ("taa_strip_kernel", "post_record_kernel", "ae_records_kernel", "cas_halo_kernel", "cas_strip_kernel",
                                           "auto_exposure_kernel")), name


# ---- allgather_taa_records over gloo ------------------------------------------------------------------------------------------

def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _record(rank, nbytes, salt):
    return torch.from_numpy(np.random.default_rng(1000 * salt + rank).integers(0, 256, nbytes, dtype=np.uint8))


def _records_worker(rank, world, port, post_bytes, taa_bytes, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from unclerenderer_amd import dist as urdist
        for mode in ("ring", "direct"):
            # both exchanges in flight together, each record packed in place in its row of the gathered buffer
            post = torch.zeros((world, post_bytes), dtype=torch.uint8)
            taa = torch.zeros((world, taa_bytes), dtype=torch.uint8)
            post[rank].copy_(_record(rank, post_bytes, 1))
            taa[rank].copy_(_record(rank, taa_bytes, 2))
            a = urdist.allgather_post_records(post, post[rank], async_op=True, mode=mode)
            b = urdist.allgather_taa_records(taa, taa[rank], async_op=True, mode=mode)
            b.wait()
            a.wait()
            assert torch.equal(post, torch.stack([_record(r, post_bytes, 1) for r in range(world)])), mode
            assert torch.equal(taa, torch.stack([_record(r, taa_bytes, 2) for r in range(world)])), mode
            # a record of its own, blocking
            taa2 = torch.zeros((world, taa_bytes), dtype=torch.uint8)
            assert urdist.allgather_taa_records(taa2, _record(rank, taa_bytes, 2), mode=mode) is None
            assert torch.equal(taa2, taa), mode
        np.save(os.path.join(out_dir, f"taa{rank}.npy"), taa.numpy())
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_allgather_taa_records_over_gloo(tmp_path, world):
    from unclerenderer_amd.hotpath import post_record_bytes, taa_record_bytes
    pb, tb = post_record_bytes(40), taa_record_bytes(40)
    mp.spawn(_records_worker, args=(world, _free_port(), pb, tb, str(tmp_path)), nprocs=world, join=True)
    want = np.stack([_record(r, tb, 2).numpy() for r in range(world)])
    for r in range(world):
        assert np.array_equal(np.load(tmp_path / f"taa{r}.npy"), want)


def test_allgather_taa_records_one_rank():
    from unclerenderer_amd import dist as urdist
    allr = torch.zeros((1, 96), dtype=torch.uint8)
    assert urdist.allgather_taa_records(allr, _record(0, 96, 2)) is None
    assert torch.equal(allr[0], _record(0, 96, 2))
