"""Lighting, Sky and the fused launch on edge and special values (tests/lighting_edges.py), on both kernels, against the oracle and
the float64 restatement: NaN, sNaN, +-Inf, +-0, subnormal, tiny-normal and >= 4 shadow texels; ShadowBias -1.5, -4, -8 and +5
(compare values > 1 at the map's border, |cmp| >= 4); compare values made exact (0, 2^-130, 0.5) against texel ladders around
them; stored depths -1, -0, 0, 2^-149, 2, +Inf, qNaN and sNaN.

Every launch proves which kernel ran: a streaming launch on a fresh context leaves its tile schedule there
(HotPath.lighting_schedule), a per-tile launch leaves none. Decisions are held to the oracle (max(1e-3, 1 fp16 ulp); its
FragileMask pixels to the bracket of its forced evaluations) and the continuous values to R1-R3 of test_gpu_accuracy.check_accuracy;
where every compare value is exact nothing is bracketed but the restatement's window-edge pixels."""
import numpy as np
import pytest

from tests import lighting_edges as E
from tests import lighting_ref64 as r64
from tests.test_gpu_accuracy import check_accuracy
from tests.util import hdr_mismatch

pytestmark = pytest.mark.gpu

W, H, SHADOW = 320, 180, 256
BAND = (36, 48)  # row0 > 0, rows


def _torch():
    import torch
    return torch


class _Kernel:
    """Launches on a context no streaming launch has used: stream=1 asserts the streaming kernel ran, stream=0 that it did not."""

    def __init__(self, urlib, stream):
        from unclerenderer_amd.hotpath import HotPath
        self.stream = stream
        self.hp = HotPath(0)

    def close(self):
        self.hp.close()

    def launch(self, form, fc, g, shadow, env, lut, row0, rows):
        from unclerenderer_amd import lib
        from unclerenderer_amd.hotpath import to_device
        hp = self.hp
        hp.set_option(lib.UR_OPT_LIGHTING_STREAM, self.stream)
        tables = hp.make_tables(to_device(shadow), hp.stage_env_cube(env, 32, 6), 32, 6, to_device(lut)) if form != "sky" else None
        keep = [to_device(a) for a in (g.A, g.B, g.C, g.depth)]
        A, B, Cc, depth = keep
        d = to_device(g.hdr if form != "sky" else self.lit_bits)
        if form == "lighting":
            hp.deferred_lighting(fc.scene, A, B, Cc, tables, d, W, H, row0, rows)
        elif form == "sky":
            hp.sky_atmosphere(fc.sky, depth, d, W, H, row0, rows)
        else:
            hp.deferred_lighting_sky(fc.scene, fc.sky, A, B, Cc, depth, tables, d, W, H, row0, rows)
        _torch().cuda.synchronize()
        return d.cpu().numpy().view(np.uint16)


def _window_fragile(fc, g, row0, rows):
    uv = r64.shadow_decisions(fc.scene, g.A, W, H, row0, rows)["uv"]
    with np.errstate(invalid="ignore"):
        return np.any((np.abs(uv) <= r64.TIE) | (np.abs(uv - 1.0) <= r64.TIE), -1).reshape(rows, W)


def _band(g, row0, rows):
    import dataclasses
    sl = slice(row0, row0 + rows)
    return dataclasses.replace(g, row0=row0, rows=rows, A=g.A[sl].copy(), B=g.B[sl].copy(), C=g.C[sl].copy(), hdr=g.hdr[sl].copy(),
                               depth=np.ascontiguousarray(g.depth[sl]).copy())


def _run(urlib, oracle, kind, streams, forms, band=False):
    from unclerenderer_amd import synth
    fc, g, shadow, exact = E.edge_frame(kind, W, H, shadow_size=SHADOW)
    row0, rows = BAND if band else (0, H)
    if band:
        g = _band(g, row0, rows)
    env, lut = synth.env_cube_procedural(32, 6), synth.brdf_lut_procedural(128, 32)
    lit, frag = oracle.deferred_lighting(fc.scene, g.A, g.B, g.C, shadow, env, 32, 6, lut, g.hdr, W, H, row0, rows, want_fragile=True)
    ref = oracle.sky_atmosphere(fc.sky, g.depth, lit, W, H, row0, rows)
    cube = r64.EnvCube(env, 32, 6)
    xl, fl = r64.deferred_lighting64(fc.scene, g.A, g.B, g.C, shadow, env, 32, 6, lut, g.hdr, W, H, row0, rows, env=cube)
    xs, fs = r64.sky_atmosphere64(fc.sky, g.depth, lit, W, H, row0, rows)
    xf, ff = r64.sky_atmosphere64(fc.sky, g.depth, xl, W, H, row0, rows)
    sky = r64.sky_drawn(fc.sky, g.depth, W, H, row0, rows)
    nv = r64.n_dot_v(fc.scene, g.A, W, H, row0, rows)
    if exact:  # every compare is exact: only the window's edges are left to rounding
        wf = _window_fragile(fc, g, row0, rows)
        frag_rule, fl = wf, wf
    else:
        frag_rule = frag
    for stream in streams:
        for form in forms:
            if form == "sky" and stream == 1:
                continue  # the sky-only launch has one kernel
            k = _Kernel(urlib, stream)
            try:
                k.lit_bits = lit
                out = k.launch(form, fc, g, shadow, env, lut, row0, rows)
                sched = k.hp.lighting_schedule()
            finally:
                k.close()
            what = f"{kind} {form} stream={stream} rows={row0}+{rows}"
            if stream == 1:
                assert sched["groups"] > 0 and sched["tiles"] == (W // 16) * ((rows + 3) // 4), f"{what}: the streaming kernel did not run ({sched})"
            else:
                assert sched["groups"] == 0, f"{what}: a streaming launch ran ({sched})"
            if form == "lighting":
                r, x, f, s, nvv = lit, xl, fl, None, nv
            elif form == "sky":
                r, x, f, s, nvv = ref, xs, fs, sky, None
            else:
                r, x, f, s, nvv = ref, xf, fl | ff, sky, np.where(sky, 1.0, nv)
            nbad, worst, badpix = hdr_mismatch(out, r, exclude=frag_rule if form != "sky" else None)
            if nbad:
                yx = np.argwhere(badpix)[:4]
                raise AssertionError(f"{what}: {nbad} channel values beyond the oracle (worst excess {worst}); pixels {yx.tolist()}")
            check_accuracy(what, out, x, f, r, None if exact or form == "sky" else frag, s, nv=nvv)


@pytest.mark.parametrize("kind", [k for k in E.EDGE_KINDS if k != "depth"])
def test_shadow_edges_on_both_kernels(urlib, oracle, hotpath, kind):
    _run(urlib, oracle, kind, streams=(1, 0), forms=("lighting", "fused"))


def test_stored_depth_specials_on_every_form(urlib, oracle, hotpath):
    _run(urlib, oracle, "depth", streams=(1, 0), forms=("lighting", "sky", "fused"))


@pytest.mark.parametrize("kind", ["texels", "bias-4", "cmp0x0p+0", "depth"])
def test_edges_on_a_row_band(urlib, oracle, hotpath, kind):
    _run(urlib, oracle, kind, streams=(1, 0), forms=("fused",), band=True)
