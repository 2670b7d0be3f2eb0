#!/usr/bin/env python3
"""Timing of the post exchange's launches on one GPU (development aid; bench.py is the contract benchmark). A single-GPU rehearsal:
the records of the other ranks are packed on the same device, and no collective is timed.

    python tools/bench_post_band.py [--sizes 4k,8k] [--rows 270,540,1080] [--iters 200] [--batches 7] [--json out.jsonl]

For each frame size and band height (N = H / rows bands; the band timed is rank 1's, which has a neighbour on both sides):
ur_pack_post_record of the band, ur_auto_exposure_records of the N records, and ur_tonemap_cas_halo of the band against
ur_tonemap_cas of the same rows of the full frame, the two timed in alternating batches. Every time is one device-event pair around a
batch of back-to-back launches (per-launch time = batch time / launches) after a warm-up, over rotating buffer sets whose bytes
exceed the 256 MiB memory-side cache, as in tools/bench_post.py. Before the times of a case are printed, the halo form's bytes are
checked equal to ur_tonemap_cas's. Per rank it prints the bytes of a record, of the RGBA8 band and of the HDR band.

The TemporalAA legs (--no-taa leaves them out) run behind them with buffer sets of their own: ur_pack_taa_record of the band, and the band
forms ur_temporal_aa_halo / ur_temporal_aa_tonemap_halo - each with the two resolved rows around the band, as a frame with CAS runs them -
against the same rows resolved by ur_temporal_aa / ur_temporal_aa_tonemap out of the full frame, in the same alternating batches, with
history (use_history = 1) and separate output images. The band forms' bytes are checked equal first. After each pair it prints halo / full
and the batch-to-batch spread (max - min of the batch times) of the full-frame form, the yardstick of "not slower".
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from tools.bench_post import CACHE_BYTES, time_batches  # noqa: E402

SIZES = {"1080p": (1920, 1080), "4k": (3840, 2160), "8k": (7680, 4320)}


def taa_legs(torch, hp, a, name, w, h, hdr, nsets, PB, TB, ev, rows_out):
    """The TemporalAA legs of one frame size (see the file comment). hdr: the current frames of the buffer sets."""
    g = torch.Generator(device="cuda").manual_seed(2)
    hist = [(torch.rand((h, w, 4), device="cuda", generator=g) * 3.0).half() for _ in range(nsets)]
    tkw = dict(exposure=0.9, gamma=2.2, exposure_ev=ev)
    for rows in (int(r) for r in a.rows.split(",")):
        if h % rows or h // rows < 3:
            continue
        n, r0 = h // rows, rows  # rank 1: a neighbour on both sides
        post = [torch.zeros((n, PB), dtype=torch.uint8, device="cuda") for _ in range(nsets)]
        taa = [torch.zeros((n, TB), dtype=torch.uint8, device="cuda") for _ in range(nsets)]
        for i in range(nsets):
            for r in (0, 1, 2):
                hp.pack_post_record(hdr[i][r * rows:(r + 1) * rows], post[i][r], w, h, r * rows, rows)
                hp.pack_taa_record(hdr[i][r * rows:(r + 1) * rows], hist[i][r * rows:(r + 1) * rows], 1, taa[i][r], w, h, r * rows, rows)
        row = lambda t, off: t[off:off + 8 * w]
        band = [x[r0:r0 + rows] for x in hdr]
        hband = [x[r0:r0 + rows] for x in hist]
        side = [dict(above2=row(t[0], 8 * w), hist_above=row(t[0], 24 * w), below2=row(t[2], 0), hist_below=row(t[2], 16 * w)) for t in taa]
        above = [row(p[0], 8 * w) for p in post]
        below = [row(p[2], 0) for p in post]
        mk = lambda shape, dt: [torch.zeros(shape, dtype=dt, device="cuda") for _ in range(nsets)]
        out_full, out_halo = mk((rows, w, 4), torch.int16), mk((rows, w, 4), torch.int16)
        ldr_full, ldr_halo = mk((rows, w), torch.int32), mk((rows, w), torch.int32)
        res = [dict(resolved_above=torch.zeros((w, 4), dtype=torch.int16, device="cuda"), resolved_below=torch.zeros((w, 4), dtype=torch.int16, device="cuda"))
               for _ in range(nsets)]
        cases = {
            "ur_pack_taa_record": lambda i: hp.pack_taa_record(band[i], hband[i], 1, taa[i][1], w, h, r0, rows),
            "ur_temporal_aa": lambda i: hp.temporal_aa(hdr[i], hband[i], out_full[i], 0.9, 1, w, h, r0, rows),
            "ur_temporal_aa_halo": lambda i: hp.temporal_aa_halo(band[i], above[i], below[i], hband[i], out_halo[i], 0.9, 1, w, h, r0, rows, **side[i], **res[i]),
            "ur_temporal_aa_tonemap": lambda i: hp.temporal_aa_tonemap(hdr[i], hband[i], out_full[i], ldr_full[i], 0.9, 1, w, h, r0, rows, **tkw),
            "ur_temporal_aa_tonemap_halo": lambda i: hp.temporal_aa_tonemap_halo(band[i], above[i], below[i], hband[i], out_halo[i], ldr_halo[i], 0.9, 1, w, h,
                                                                                 r0, rows, **side[i], **res[i], **tkw),
        }
        for k in ("ur_temporal_aa", "ur_temporal_aa_halo"):
            cases[k](0)
        torch.cuda.synchronize()
        assert torch.equal(out_full[0], out_halo[0]), f"{name}/{rows}: ur_temporal_aa_halo differs from ur_temporal_aa"
        out_halo[0].zero_()
        for k in ("ur_temporal_aa_tonemap", "ur_temporal_aa_tonemap_halo"):
            cases[k](0)
        torch.cuda.synchronize()
        assert torch.equal(out_full[0], out_halo[0]) and torch.equal(ldr_full[0], ldr_halo[0]), f"{name}/{rows}: ur_temporal_aa_tonemap_halo differs"
        times = {k: [] for k in cases}
        for _ in range(a.batches):
            for k, fn in cases.items():
                times[k] += time_batches(torch, fn, nsets, a.iters, 1, warm=3)
        per_rank = {"post_record": PB, "taa_record": TB, "exchanged": PB + TB, "hdr_band": w * rows * 8}
        print(f"{name:>5} rows {rows:5d} (N = {n:2d})  TemporalAA; bytes per rank: post record {PB / 1e3:.1f} KB + TAA record {TB / 1e3:.1f} KB = "
              f"{(PB + TB) / 1e3:.1f} KB exchanged, HDR band {w * rows * 8 / 1e6:.2f} MB", flush=True)
        for k, t in times.items():
            med = float(np.median(t))
            print(f"      {k:<28} {med:8.2f} us  [{min(t):.2f}, {max(t):.2f}]", flush=True)
            rows_out.append({"size": name, "w": w, "h": h, "rows": rows, "ranks": n, "op": k, "us_median": round(med, 2), "us_min": round(min(t), 2),
                             "us_max": round(max(t), 2), "sets": nsets, **per_rank})
        for full, halo in (("ur_temporal_aa", "ur_temporal_aa_halo"), ("ur_temporal_aa_tonemap", "ur_temporal_aa_tonemap_halo")):
            tf, th = float(np.median(times[full])), float(np.median(times[halo]))
            print(f"      {halo} / {full} {th / tf:.4f}  ({th - tf:+.2f} us; spread of the full-frame form {max(times[full]) - min(times[full]):.2f} us)", flush=True)
        del post, taa, band, hband, side, above, below, out_full, out_halo, ldr_full, ldr_halo, res
    del hist


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4k,8k")
    ap.add_argument("--rows", default="270,540,1080")
    ap.add_argument("--iters", type=int, default=200, help="launches per timed batch")
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--json", default="", help="also append one JSON line per measurement to this file")
    ap.add_argument("--no-taa", action="store_true", help="leave out the TemporalAA legs")
    ap.add_argument("--only-taa", action="store_true", help="only the TemporalAA legs")
    a = ap.parse_args()
    import torch
    from unclerenderer_amd.hotpath import HotPath, post_record_bytes, taa_record_bytes
    assert torch.cuda.is_available(), "bench_post_band needs a GPU"
    hp = HotPath(0)
    rows_out = []
    for name in a.sizes.split(","):
        w, h = SIZES[name]
        nsets = max(2, -(-3 * CACHE_BYTES // (w * h * 8)))
        g = torch.Generator(device="cuda").manual_seed(1)
        hdr = [(torch.rand((h, w, 4), device="cuda", generator=g) * 3.0).half() for _ in range(nsets)]
        ev = torch.zeros(1, device="cuda")
        hp.auto_exposure(hdr[0], ev, w, h)
        kw = dict(exposure=0.9, gamma=2.2, exposure_ev=ev, sharpness=0.5)
        B = post_record_bytes(w)
        for rows in (int(r) for r in a.rows.split(",")):
            if h % rows or a.only_taa:
                continue
            n, r0 = h // rows, rows  # rank 1
            recs = [torch.zeros((n, B), dtype=torch.uint8, device="cuda") for _ in range(nsets)]
            for i in range(nsets):
                for r in range(n):
                    hp.pack_post_record(hdr[i][r * rows:(r + 1) * rows], recs[i][r], w, h, r * rows, rows)
            out_full = [torch.zeros((rows, w), dtype=torch.int32, device="cuda") for _ in range(nsets)]
            out_halo = [torch.zeros((rows, w), dtype=torch.int32, device="cuda") for _ in range(nsets)]
            band = [x[r0:r0 + rows] for x in hdr]
            above = [x[0, 8 * w:16 * w] for x in recs]
            below = [x[2, :8 * w] if n > 2 else None for x in recs]
            ev_rec = torch.zeros(1, device="cuda")
            hp.auto_exposure_records(recs[0], n, ev_rec, w, h)
            hp.tonemap_cas(hdr[0], out_full[0], w, h, row0=r0, rows=rows, **kw)
            hp.tonemap_cas_halo(band[0], above[0], below[0], out_halo[0], w, h, r0, rows, **kw)
            torch.cuda.synchronize()
            assert torch.equal(out_full[0], out_halo[0]), f"{name}/{rows}: ur_tonemap_cas_halo differs from ur_tonemap_cas"
            assert torch.equal(ev, ev_rec), f"{name}/{rows}: ur_auto_exposure_records differs from ur_auto_exposure"
            cases = {
                "ur_pack_post_record": lambda i: hp.pack_post_record(band[i], recs[i][1], w, h, r0, rows),
                "ur_auto_exposure_records": lambda i: hp.auto_exposure_records(recs[i], n, ev_rec, w, h),
                "ur_tonemap_cas": lambda i: hp.tonemap_cas(hdr[i], out_full[i], w, h, row0=r0, rows=rows, **kw),
                "ur_tonemap_cas_halo": lambda i: hp.tonemap_cas_halo(band[i], above[i], below[i], out_halo[i], w, h, r0, rows, **kw),
            }
            times = {k: [] for k in cases}
            for _ in range(a.batches):  # alternating batches: the two strip forms see the same conditions
                for k, fn in cases.items():
                    times[k] += time_batches(torch, fn, nsets, a.iters, 1, warm=3)
            per_rank = {"record": B, "rgba8_band": w * rows * 4, "hdr_band": w * rows * 8}
            print(f"{name:>5} rows {rows:5d} (N = {n:2d})  bytes per rank: record {B / 1e3:.1f} KB, RGBA8 band {w * rows * 4 / 1e6:.2f} MB, "
                  f"HDR band {w * rows * 8 / 1e6:.2f} MB", flush=True)
            for k, t in times.items():
                med = float(np.median(t))
                print(f"      {k:<26} {med:8.2f} us  [{min(t):.2f}, {max(t):.2f}]", flush=True)
                rows_out.append({"size": name, "w": w, "h": h, "rows": rows, "ranks": n, "op": k, "us_median": round(med, 2), "us_min": round(min(t), 2),
                                 "us_max": round(max(t), 2), "sets": nsets, **per_rank})
            tf, th = float(np.median(times["ur_tonemap_cas"])), float(np.median(times["ur_tonemap_cas_halo"]))
            print(f"      halo / full {th / tf:.4f}  ({th - tf:+.2f} us)", flush=True)
            del recs, out_full, out_halo, band, above, below
        if not a.no_taa:
            taa_legs(torch, hp, a, name, w, h, hdr, nsets, B, taa_record_bytes(w), ev, rows_out)
        del hdr
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "a") as f:
            for r in rows_out:
                f.write(json.dumps(r) + "\n")
    hp.close()


if __name__ == "__main__":
    main()
