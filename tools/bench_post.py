#!/usr/bin/env python3
"""Timing of the post-chain launches on one GPU (development aid; bench.py is the contract benchmark).

    python tools/bench_post.py [--sizes 1080p,4k,8k] [--iters 200] [--batches 7] [--legs post,taa] [--json out.jsonl]

For each frame size: ur_tonemap, ur_cas, ur_tonemap + ur_cas back to back, ur_tonemap_cas and ur_auto_exposure, each timed with
one device-event pair around a batch of back-to-back launches (per-launch time = batch time / launches), after a warm-up, over
enough rotating buffer sets that a batch's bytes exceed the 256 MiB memory-side cache. Bytes per pixel: Tonemap 12
(8 read + 4 written), CAS 8 (4 + 4), the pair 20, fused 12 (8 + 4). Before any time of a size is printed, the fused output is
checked byte-equal to the two launches. The fraction is bytes / time over 8 TB/s (the HBM peak of MI355X).
The byte counts above are what must cross HBM at least. The CAS strip kernels (csrc/post.hip) also load the two halo rows of every
STRIP_ROWS-row strip that the neighbouring strips load too, so they issue more: CAS 4 * 10 / 8 + 4 = 9 B/pixel, fused 8 * 10 / 8 + 4 = 14;
whether those repeated rows come from L2 / the memory-side cache or from HBM is not measured. Both figures are printed.

The "taa" leg: ur_temporal_aa (24 B/pixel), ur_temporal_aa + ur_tonemap back to back (36) and ur_temporal_aa_tonemap (28; also with
UR_OPT_TAA_TONEMAP_HISTORY_STORE = 1, the plain history store), over the same kind of rotating cold buffer sets, in the same process.
Its batches ALTERNATE between the cases (pair, fused, fused with the plain store, pair, ...), so that a drift of the clocks during the
run lands on all of them alike; the median over the batches of each case is reported, and the last line of a size gives the fused
launch against the pair with the pair's own batch-to-batch spread. The strip kernel loads 10 current rows per 8 output rows.

The "debugprint" leg (--legs debugprint): ur_debug_print_draw with the built-in font on rotating cold R8G8B8A8 images, with the two
stats lines ("FRUSTUM 12345" / "OCCLUDE 67890", 26 entries) and with a full buffer of 4096 entries spread over the frame. The
launch reads and writes only the 64 x 64 tiles the text touches, so no byte count is given: the claim to check is that the two stats
lines cost the same at 4K and 8K (a launch, not a pass over the frame). The last line of the leg prints that ratio.
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

SIZES = {"1080p": (1920, 1080), "4k": (3840, 2160), "8k": (7680, 4320)}
PEAK_BPS = 8e12
STRIP_ROWS = 8  # output rows per wave of csrc/post.hip's strip kernels (kRows): kRows + 2 input rows are loaded per strip
CACHE_BYTES = 256 << 20


def time_batches(torch, fn, nsets, iters, batches, warm=10):
    for k in range(warm):
        fn(k % nsets)
    torch.cuda.synchronize()
    out = []
    for _ in range(batches):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for k in range(iters):
            fn(k % nsets)
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / iters)
    return out


def time_alternating(torch, fns, nsets, iters, batches, warm=10):
    """time_batches for several launches at once: batch b of every case before batch b + 1 of any."""
    for fn in fns:
        for k in range(warm):
            fn(k % nsets)
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(batches):
        for t, fn in zip(out, fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for k in range(iters):
                fn(k % nsets)
            b.record()
            torch.cuda.synchronize()
            t.append(a.elapsed_time(b) * 1e3 / iters)
    return out


def debugprint_leg(torch, hp, a, report):
    from unclerenderer_amd import hostmath
    from unclerenderer_amd.hotpath import debug_print_buffer, to_device
    atlas, glyphs, first, count = hostmath.debug_font()
    d_atlas, d_glyphs = torch.from_numpy(atlas).cuda(), to_device(glyphs)
    stats_med = {}
    for name in a.sizes.split(","):
        w, h = SIZES[name]
        nsets = max(2, -(-3 * CACHE_BYTES // (w * h * 4)))
        g = torch.Generator(device="cuda").manual_seed(2)
        img = [torch.randint(-2 ** 31, 2 ** 31 - 1, (h, w), dtype=torch.int32, device="cuda", generator=g) for _ in range(nsets)]
        two = debug_print_buffer()
        hp.debug_print_stats(to_device(np.array([12345, 67890], np.uint32)), two)
        full = debug_print_buffer()
        rng = np.random.default_rng(3)
        for _ in range(4096 // 16):  # 256 strings of 16 characters all over the frame
            hp.debug_print_text(full, int(rng.integers(0, w - 128)), int(rng.integers(8, h)), bytes(int(c) for c in rng.integers(33, 96, 16)),
                                int(rng.integers(0, 1 << 32)))
        torch.cuda.synchronize()
        assert int(two[0]) == 26 and int(full[0]) == 4096

        def draw(buf):
            return lambda i: hp.debug_print_draw(buf, d_glyphs, d_atlas, img[i], w, h, first_char=first, char_count=count)

        ts = time_alternating(torch, [draw(two), draw(full)], nsets, a.iters, a.batches)
        stats_med[name] = report(name, w, h, "debug_draw/2 lines", 0, 0, ts[0], nsets)
        report(name, w, h, "debug_draw/4096", 0, 0, ts[1], nsets)
        del img
        torch.cuda.empty_cache()
    if "4k" in stats_med and "8k" in stats_med:
        print(f"debug_draw, two stats lines: 8K / 4K = {stats_med['8k'] / stats_med['4k']:.2f} ({stats_med['4k']:.2f} us -> {stats_med['8k']:.2f} us)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1080p,4k,8k")
    ap.add_argument("--iters", type=int, default=200, help="launches per timed batch")
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--sharpness", type=float, default=0.5)
    ap.add_argument("--legs", default="post,taa", help="post: Tonemap / CAS / AutoExposure; taa: TemporalAA + Tonemap against the fused launch; "
                                                       "debugprint: the GpuDebugPrint draw")
    ap.add_argument("--json", default="", help="also append one JSON line per measurement to this file")
    a = ap.parse_args()
    import torch
    from unclerenderer_amd import lib
    from unclerenderer_amd.hotpath import HotPath
    assert torch.cuda.is_available(), "bench_post needs a GPU"
    hp = HotPath(0)
    rows_out = []
    legs = set(a.legs.split(","))

    def report(name, w, h, label, bpp, issued, t, nsets):
        px = w * h
        med = float(np.median(t))
        r = {"size": name, "w": w, "h": h, "op": label, "bytes": px * bpp, "us_median": round(med, 2), "us_min": round(min(t), 2),
             "us_max": round(max(t), 2), "frac_8TBps": round(px * bpp / (med * 1e-6) / PEAK_BPS, 3) if bpp else None,
             "issued_bytes": int(px * issued), "issued_frac_8TBps": round(px * issued / (med * 1e-6) / PEAK_BPS, 3) if bpp else None, "sets": nsets}
        rows_out.append(r)
        frac = f"{r['frac_8TBps']:.3f}" if bpp else "  -  "
        ifrac = f"{r['issued_frac_8TBps']:.3f}" if bpp else "  -  "
        print(f"{name:>5} {label:<18} {px * bpp / 1e6:8.1f} MB  {med:8.2f} us  [{min(t):.2f}, {max(t):.2f}]  {frac} of 8 TB/s"
              f"  (issued {px * issued / 1e6:6.1f} MB: {ifrac})", flush=True)
        return med
    for name in a.sizes.split(",") if legs & {"post", "taa"} else []:
        w, h = SIZES[name]
        px = w * h
        set_bytes = px * (8 + 4 + 4 + 4)
        nsets = max(2, -(-3 * CACHE_BYTES // set_bytes))
        g = torch.Generator(device="cuda").manual_seed(1)
        hdr = [(torch.rand((h, w, 4), device="cuda", generator=g) * 3.0).half() for _ in range(nsets)]
        ldr = [torch.zeros((h, w), dtype=torch.int32, device="cuda") for _ in range(nsets)]
        out = [torch.zeros((h, w), dtype=torch.int32, device="cuda") for _ in range(nsets)]
        fused = [torch.zeros((h, w), dtype=torch.int32, device="cuda") for _ in range(nsets)]
        ev = torch.zeros(1, device="cuda")
        hp.auto_exposure(hdr[0], ev, w, h)
        kw = dict(exposure=0.9, gamma=2.2, exposure_ev=ev)
        # the fused launch must give the two launches' bytes at this size
        hp.tonemap(hdr[0], ldr[0], w, h, **kw)
        hp.cas(ldr[0], out[0], w, h, sharpness=a.sharpness)
        hp.tonemap_cas(hdr[0], fused[0], w, h, sharpness=a.sharpness, **kw)
        torch.cuda.synchronize()
        assert torch.equal(out[0], fused[0]), f"{name}: ur_tonemap_cas differs from ur_tonemap + ur_cas"

        def two(i):
            hp.tonemap(hdr[i], ldr[i], w, h, **kw)
            hp.cas(ldr[i], out[i], w, h, sharpness=a.sharpness)

        halo = (STRIP_ROWS + 2) / STRIP_ROWS
        # (label, DRAM-floor bytes per pixel, bytes per pixel the launch issues, launch)
        cases = [
            ("ur_tonemap", 12, 12, lambda i: hp.tonemap(hdr[i], ldr[i], w, h, **kw)),
            ("ur_cas", 8, 4 * halo + 4, lambda i: hp.cas(ldr[i], out[i], w, h, sharpness=a.sharpness)),
            ("ur_tonemap+ur_cas", 20, 12 + 4 * halo + 4, two),
            ("ur_tonemap_cas", 12, 8 * halo + 4, lambda i: hp.tonemap_cas(hdr[i], fused[i], w, h, sharpness=a.sharpness, **kw)),
            ("ur_auto_exposure", 0, 0, lambda i: hp.auto_exposure(hdr[i], ev, w, h)),
        ]
        for label, bpp, issued, fn in cases if "post" in legs else []:
            report(name, w, h, label, bpp, issued, time_batches(torch, fn, nsets, a.iters, a.batches), nsets)
        if "taa" in legs:
            hist = [(torch.rand((h, w, 4), device="cuda", generator=g) * 3.0).half() for _ in range(nsets)]
            res = [torch.zeros((h, w, 4), dtype=torch.float16, device="cuda") for _ in range(nsets)]
            res1 = [torch.zeros((h, w, 4), dtype=torch.float16, device="cuda") for _ in range(nsets)]
            # the fused launch must give the two launches' bytes at this size, under either store hint
            hp.temporal_aa(hdr[0], hist[0], res[0], 0.9, True, w, h)
            hp.tonemap(res[0], ldr[0], w, h, **kw)
            for plain in (0, 1):
                hp.set_option(lib.UR_OPT_TAA_TONEMAP_HISTORY_STORE, plain)
                res1[0].zero_()
                fused[0].zero_()
                hp.temporal_aa_tonemap(hdr[0], hist[0], res1[0], fused[0], 0.9, True, w, h, **kw)
                torch.cuda.synchronize()
                assert torch.equal(res1[0].view(torch.int16), res[0].view(torch.int16)) and torch.equal(fused[0], ldr[0]), \
                    f"{name}: ur_temporal_aa_tonemap (store {plain}) differs from ur_temporal_aa + ur_tonemap"

            def pair(i):
                hp.temporal_aa(hdr[i], hist[i], res[i], 0.9, True, w, h)
                hp.tonemap(res[i], ldr[i], w, h, **kw)

            def one(plain):
                def fn(i):
                    hp.set_option(lib.UR_OPT_TAA_TONEMAP_HISTORY_STORE, plain)
                    hp.temporal_aa_tonemap(hdr[i], hist[i], res1[i], fused[i], 0.9, True, w, h, **kw)
                return fn

            taa_cases = [
                ("ur_temporal_aa", 24, 8 * halo + 16, lambda i: hp.temporal_aa(hdr[i], hist[i], res[i], 0.9, True, w, h)),
                ("ur_taa+ur_tonemap", 36, 8 * halo + 16 + 12, pair),
                ("ur_taa_tonemap", 28, 8 * halo + 20, one(0)),
                ("ur_taa_tonemap/pl", 28, 8 * halo + 20, one(1)),
            ]
            ts = time_alternating(torch, [c[3] for c in taa_cases], nsets, a.iters, a.batches)
            hp.set_option(lib.UR_OPT_TAA_TONEMAP_HISTORY_STORE, 0)
            med = [report(name, w, h, label, bpp, issued, t, nsets) for (label, bpp, issued, _), t in zip(taa_cases, ts)]
            spread = max(ts[1]) - min(ts[1])
            print(f"{name:>5} fused / pair = {med[2] / med[1]:.3f} (28 / 36 = {28 / 36:.3f}); pair - fused = {med[1] - med[2]:.2f} us, the pair's batch-to-batch "
                  f"spread {spread:.2f} us; plain history store / write-through nontemporal = {med[3] / med[2]:.3f}", flush=True)
            del hist, res, res1
        del hdr, ldr, out, fused
        torch.cuda.empty_cache()
    if "debugprint" in legs:
        debugprint_leg(torch, hp, a, report)
    if a.json:
        with open(a.json, "a") as f:
            for r in rows_out:
                f.write(json.dumps(r) + "\n")
    hp.close()


if __name__ == "__main__":
    main()
