"""bench.dump_outputs on host tensors: the files it writes, their dtypes, the 64 MB limit at the bench's 4K frame, and the
fixed seeded samples (whole frame rows, HZB texels with their offsets) taken where an output does not fit."""
import numpy as np
import torch

import bench


def _inputs(w, h, hzb_texels, ldr):
    g = torch.Generator().manual_seed(7)
    hdr = (torch.rand((h, w, 4), generator=g) * 4.0).to(torch.float16).view(torch.int16)
    ldr_t = torch.randint(-2**31, 2**31 - 1, (h, w), dtype=torch.int32, generator=g) if ldr else None
    hzb = torch.rand(hzb_texels, generator=g)
    args = torch.arange(25 * 16, dtype=torch.int32).reshape(25, 16)
    vis = torch.tensor(list(range(20)) + [-1] * 5, dtype=torch.int32)
    return hdr, ldr_t, hzb, args, vis, torch.tensor([20], dtype=torch.int32)


def test_dump_at_4k_fits_and_keeps_the_values(tmp_path):
    hdr, _, hzb, args, vis, cnt = _inputs(3840, 2160, 2764928, False)  # the bench frame: 4K, an 11-mip HZB of 2764928 texels
    shapes = bench.dump_outputs(tmp_path, hdr, None, hzb, args, vis, cnt)
    files = sorted(p.name for p in tmp_path.iterdir())
    assert files == sorted(f"{n}.npy" for n in shapes) == sorted(["hdr.npy", "frame_rows.npy", "hzb.npy", "indirect_args.npy",
                                                                  "visible_indices.npy", "visible_count.npy"])
    assert sum((tmp_path / f).stat().st_size for f in files) <= bench.DUMP_MAX_BYTES
    assert all(np.load(tmp_path / f).dtype in (np.float32, np.float64) for f in files)
    rows = np.load(tmp_path / "frame_rows.npy").astype(np.int64)
    assert rows.size == bench.DUMP_FRAME_BYTES // (3840 * 16) < 2160 and np.all(np.diff(rows) > 0)
    assert np.array_equal(np.load(tmp_path / "hdr.npy"), hdr.numpy().view(np.float16)[rows].astype(np.float32))
    assert np.array_equal(np.load(tmp_path / "hzb.npy"), hzb.numpy())  # 10.5 MB: whole
    assert np.array_equal(np.load(tmp_path / "indirect_args.npy"), args.numpy().astype(np.float64))
    assert np.array_equal(np.load(tmp_path / "visible_indices.npy"), np.arange(20, dtype=np.float64))
    assert np.load(tmp_path / "visible_count.npy").tolist() == [20.0]


def test_dump_samples_are_fixed_and_index_the_outputs(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_FRAME_BYTES", 10 * 64 * 32)  # ten rows of HDR + LDR at width 64
    monkeypatch.setattr(bench, "DUMP_HZB_BYTES", 12 * 300)       # 300 texels with their offsets
    hdr, ldr, hzb, args, vis, cnt = _inputs(64, 48, 1000, True)
    for d in ("a", "b"):
        bench.dump_outputs(tmp_path / d, hdr, ldr, hzb, args, vis, cnt)
    for f in (tmp_path / "a").iterdir():
        assert np.array_equal(np.load(f), np.load(tmp_path / "b" / f.name)), f.name
    rows = np.load(tmp_path / "a" / "frame_rows.npy").astype(np.int64)
    assert rows.size == 10 and np.all(np.diff(rows) > 0) and rows[-1] < 48
    assert np.array_equal(np.load(tmp_path / "a" / "ldr.npy"), ldr.numpy().view(np.uint8).reshape(48, 64, 4)[rows].astype(np.float32))
    idx = np.load(tmp_path / "a" / "hzb_index.npy").astype(np.int64)
    assert idx.size == 300 and np.all(np.diff(idx) > 0) and idx[-1] < 1000
    assert np.array_equal(np.load(tmp_path / "a" / "hzb.npy"), hzb.numpy()[idx])
