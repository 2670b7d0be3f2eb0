"""The decision forms of the lighting kernels (csrc/lighting.hip, csrc/lighting_tiled.hip) held to the shaders' semantics on edge and special values, on the CPU: fp32 emulations
of each form (tests/lighting_edges.py) against LESS_EQUAL / GREATER_EQUAL, the mutant table that shows every former form and every
plain mutant caught, the edge frames' generators, and the oracle against the float64 restatement on those frames.
tests/test_gpu_lighting_edges.py runs the same frames through the kernels."""
import numpy as np
import pytest

from tests import lighting_edges as E
from tests import lighting_ref64 as r64
from tests.util import hdr_mismatch


def _differences(form, pts, ref):
    return [(a, b) for a, b in pts if form(a, b) != ref(a, b)]


def test_fixed_tap_forms_equal_less_equal_everywhere():
    pts = E.tap_points()
    for name in E.FIXED_TAP_FORMS:
        bad = _differences(E.TAP_FORMS[name], pts, E.tap_hlsl)
        assert not bad, f"{name}: {len(bad)} of {len(pts)} (cmp, t) pairs differ from cmp <= t, e.g. {bad[:4]}"


def test_neg_pred_big_is_the_scaled_predecessor():
    """The streaming kernel's fma(|cmp|, 2^-24 + 2^-47, -cmp) is -pred(cmp) exactly over le_step's range, powers of two,
    both signs and the range's ends included."""
    rng = np.random.default_rng(3)
    vals = [2.0 ** -100, 2.0 - 2.0 ** -23, 1.0, 0.5, 0.75, 1.5, 2.0 ** -99 * 1.75]
    vals += [float(np.float32(v)) for v in np.exp2(rng.uniform(-100, 1, 300)) * rng.uniform(1, 2, 300)]
    for c in [v for v in vals if E.cmp_step_exact(v)]:
        for x in (c, -c):
            assert E.neg_pred_big(x) == -E.pred32(x) * 2.0 ** 126, x


def test_every_former_form_and_mutant_is_caught():
    """The mutant table: each former kernel form (H1-H5) and each plain mutant changes a decision on some generated point."""
    pts = E.tap_points()
    rows = []
    for name, form in E.TAP_FORMS.items():
        bad = _differences(form, pts, E.tap_hlsl)
        kinds = set()
        for c, t in bad:
            if np.isnan(t) or np.isnan(c):
                kinds.add("H1 NaN")
            elif np.isfinite(c) and abs(c) >= 4:
                kinds.add("H2 |cmp|>=4")
            elif 0 < abs(t - c) < 2.0 ** -126:
                kinds.add("H5 |t-cmp|<2^-126")
            else:
                kinds.add("other")
        rows.append((name, len(bad), sorted(kinds)))
    cmps = [0.5, 1.0, float(np.nextafter(np.float32(1.0), np.float32(2.0))), 1.5, 5.0, float("nan")]
    for name, form in E.BORDER_FORMS.items():
        rows.append((name, sum(form(c) != E.border_hlsl(c) for c in cmps), ["H4 cmp>1"] if form is E.border_always_passes else []))
    sky_pts = [(s, d) for s in (0.01, 0.5, 0.3) for d in [E.f32(b) for b in E.SPECIAL_DEPTH_BITS] + E.ulp_ladder(s, 4)]
    for name, form in E.SKY_FORMS.items():
        bad = _differences(form, sky_pts, E.sky_hlsl)
        rows.append((name, len(bad), ["H3 depth<0"] if any(d < 0 for _, d in bad) else []))
    rows.append(("mutant window <", sum(E.window_strict(u) != E.window_hlsl(u) for u in (0.0, 1.0, 0.5)), []))
    print("\nform / mutant                               points differing  from")
    for name, n, kinds in rows:
        print(f"  {name:42s} {n:8d}  {', '.join(kinds)}")
    got = {name: (n, kinds) for name, n, kinds in rows}
    assert set(got["gt_step (streaming, before)"][1]) >= {"H1 NaN", "H2 |cmp|>=4", "H5 |t-cmp|<2^-126"}
    assert "H5 |t-cmp|<2^-126" in got["step_le (per-tile, before)"][1]
    assert got["border always passes (streaming, before)"][1] == ["H4 cmp>1"]
    assert got["squared (streaming, before)"][1] == ["H3 depth<0"]
    for name in ("mutant <", "mutant NaN passes", "mutant >", "mutant window <"):
        assert got[name][0] > 0, f"{name} is not caught"
    for name in E.FIXED_TAP_FORMS + ("border compared", "sign-aware squared (streaming)"):
        assert got[name][0] == 0, f"{name} differs from the shader on {got[name][0]} points"


def test_ladders_straddle_their_threshold():
    for c in (0.5, 2.0 ** -110, 1.0, -0.5, 5.0):
        lad = E.ulp_ladder(c, 12)
        assert lad[0] == c and len(set(lad)) == len(lad) == 27
        assert sum(t >= c for t in lad) == 14 and sum(t < c for t in lad) == 13  # 0 and +1..+2^12 pass, -1..-2^12 fail
        assert E.pred32(c) in lad and E.tap_hlsl(c, E.pred32(c)) == 0.0 and E.tap_hlsl(c, c) == 1.0


def _frame_oracle_and_r64(oracle, kind, w=160, h=96):
    from unclerenderer_amd import synth
    fc, g, shadow, exact = E.edge_frame(kind, w, h, shadow_size=128)
    env, lut = synth.env_cube_procedural(32, 6), synth.brdf_lut_procedural(128, 32)
    lit, frag = oracle.deferred_lighting(fc.scene, g.A, g.B, g.C, shadow, env, 32, 6, lut, g.hdr, w, h, want_fragile=True)
    ref = oracle.sky_atmosphere(fc.sky, g.depth, lit, w, h)
    xl, fl = r64.deferred_lighting64(fc.scene, g.A, g.B, g.C, shadow, env, 32, 6, lut, g.hdr, w, h)
    xf, ff = r64.sky_atmosphere64(fc.sky, g.depth, xl, w, h)
    return fc, g, shadow, exact, lit, frag, ref, xl, fl, xf, ff


@pytest.mark.parametrize("kind", E.EDGE_KINDS)
def test_edge_frames_reach_their_edges(kind):
    """Each generated frame holds the decisions it is meant to: lit in-window pixels whose 3x3 block reads a special texel or
    the border with cmp > 1 or |cmp| >= 4, exact compare values, or stored depths that are special on sky-test pixels."""
    w, h = 160, 96
    fc, g, shadow, exact = E.edge_frame(kind, w, h, shadow_size=128)
    d = r64.shadow_decisions(fc.scene, g.A, w, h)
    lit = d["inside"]
    assert lit.sum() > 100, "too few pixels inside the shadow window"
    if kind == "depth":
        sp = np.ascontiguousarray(g.depth, np.float32).view(np.uint32)
        for b in E.SPECIAL_DEPTH_BITS:
            assert (sp == b).sum() > 10, hex(b)
        return
    n = shadow.shape[0]
    rr, cc = np.meshgrid(np.arange(3), np.arange(3), indexing="ij")
    i = d["ia"][lit, None, None] + cc
    j = d["ja"][lit, None, None] + rr
    out = (i < 0) | (j < 0) | (i >= n) | (j >= n)
    t = shadow[np.clip(j, 0, n - 1), np.clip(i, 0, n - 1)].astype(np.float64)
    cmp = d["cmp64"][lit]
    if exact:
        T = float(fc.scene.LightViewProjection[14])
        assert np.all(cmp == T), "the compare value is not exactly T"
        assert (t == cmp[:, None, None]).any() and (t == E.pred32(T)).any() and np.isnan(t).any()
        return
    assert np.isnan(t[~out]).any() and np.isinf(t[~out]).any(), "no lit pixel reads a NaN or an Inf texel"
    assert out.any(axis=(1, 2)).sum() > 10, "no lit pixel's footprint crosses the map's border"
    if kind.startswith("bias"):
        b = float(kind[4:])
        if b <= -4:
            assert (cmp >= 4).mean() > 0.5
        elif b > 0:
            assert (cmp <= -4).mean() > 0.5
        else:
            assert (cmp > 1).mean() > 0.5 and (out.any(axis=(1, 2)) & (cmp > 1)).sum() > 10


@pytest.mark.parametrize("kind", E.EDGE_KINDS)
def test_oracle_agrees_with_restatement_on_edge_frames(oracle, kind):
    """The fp32 oracle and the float64 restatement make the same decisions on the special sets: every channel within
    max(1e-3, 1 fp16 ulp) outside the restatement's fragile pixels, NaN-ness equal."""
    fc, g, shadow, exact, lit, frag, ref, xl, fl, xf, ff = _frame_oracle_and_r64(oracle, kind)
    for what, bits, x, f in (("lighting", lit, xl, fl), ("lighting+sky", ref, xf, fl | ff)):
        r = r64.round16(x).astype(np.float16).view(np.uint16)
        skip = f if not exact else np.zeros_like(f)
        nbad, worst, _ = hdr_mismatch(bits, r, exclude=skip)
        assert nbad == 0, f"{kind} {what}: {nbad} oracle values beyond max(1e-3, 1 ulp) of the restatement (worst {worst})"
        assert (np.isnan(half(bits)) == np.isnan(x)).all(), f"{kind} {what}: NaN-ness differs"


def half(bits):
    return np.ascontiguousarray(bits, np.uint16).view(np.float16).astype(np.float64)
