"""The lighting and sky kernels held to the float64 restatement (tests/lighting_ref64.py), on top of the max(1e-3, 1 fp16 ulp)
parity with the oracle that every HDR test asserts. With x the exact value of a channel, u(x) the fp16 ulp at round16(x) and
e = (value - x) / u(x):

  R1 faithful:        |e_gpu| <= 1; where the oracle itself is farther than one ulp, |e_gpu| <= |e_oracle| + 1;
  R2 misrounding:     the share of values != round16(x) is at most twice the oracle's on the same inputs, plus 1e-3;
  R3 no bias:         the mean of e_gpu over the finite RGB values is within +-0.02, and so is it over the values below 0.25
                      and over the sky's pixels (each over at least 10^4 values: 0.02 is then > 5 standard errors of an
                      unbiased rounding, sigma ~ 0.29 per value).

The oracle's FragileMask pixels (a shadow compare within 1e-5 of flipping in fp32) keep the bracket rule of tests/util.py; pixels
that only the restatement flags (fragile64: a decision within 1e-5 of its threshold in float64) are held to hdr_mismatch."""
import numpy as np
import pytest

from tests import lighting_ref64 as r64
from tests.util import hdr_mismatch

pytestmark = pytest.mark.gpu

R3_MIN_VALUES = 10_000
# Named ill-conditioning (the only values R1 may miss): pixels whose view-space N.V is below GRAZING_NV. There the specular term
# is proportional to N.V (G ~ N.V / k and the 1e-4 clamp of 4 N.L N.V holds the denominator still) while N.V itself, a
# difference of products of unit vectors, carries an fp32 error of ~1e-7 absolute: a relative error of 1e-7 / N.V in that term
# (5e-3 at N.V = 2e-5, several fp16 ulps). At most GRAZING_MAX_SHARE of the measured values may be such exceptions.
GRAZING_NV = 1e-3
GRAZING_MAX_SHARE = 1e-4


def _torch():
    import torch
    return torch


def check_accuracy(what, gpu_bits, x, f64, ref_bits=None, frag=None, sky=None, oracle_misround=None, nv=None):
    """R1-R3 of `gpu_bits` against the exact `x`; the oracle's `ref_bits` (same pixels) scales R1 and R2 and carries the old
    parity rule. Pixels in `frag` (the oracle's FragileMask) or `f64` are left out of R1-R3. Without `ref_bits` (a pixel sample
    the oracle cannot evaluate), R1 is |e| <= 1 and R2 is scaled by `oracle_misround`, the oracle's rate on other pixels of the
    same frame. `nv`: the pixels' N.V (lighting_ref64.n_dot_v) for the grazing allowance; None allows nothing."""
    f64 = np.asarray(f64, bool)
    skip = f64.copy()
    if ref_bits is not None:
        frag_b = np.zeros(f64.shape, bool) if frag is None else np.asarray(frag, bool)
        skip |= frag_b
        nbad, worst, _ = hdr_mismatch(gpu_bits, ref_bits, exclude=frag)
        assert nbad == 0, f"{what}: {nbad} channel values beyond max(1e-3, 1 ulp) of the oracle (worst excess {worst})"
        only64 = f64 & ~frag_b
        if only64.any():
            nbad, worst, _ = hdr_mismatch(gpu_bits[only64], ref_bits[only64])
            assert nbad == 0, f"{what}: {nbad} fragile64 channel values beyond max(1e-3, 1 ulp) of the oracle (worst {worst})"
    m = r64.measure(gpu_bits, x, skip, sky)
    assert m["nan_mismatch"] == 0, f"{what}: {m['nan_mismatch']} values whose NaN-ness differs from the exact value's"
    e_ref = None
    if ref_bits is not None:
        mr = r64.measure(ref_bits, x, skip)
        e_ref = mr["e"]
        r2_bound = 2 * mr["misround"] + 1e-3
    else:
        r2_bound = 2 * oracle_misround + 1e-3
    bad = r64.r1_violations(m["e"], e_ref)
    if nv is not None:
        grazing = bad & (np.abs(np.asarray(nv))[..., None] < GRAZING_NV) & (np.arange(bad.shape[-1]) < 3)
        assert grazing.sum() <= GRAZING_MAX_SHARE * m["n"], f"{what}: {int(grazing.sum())} grazing values miss R1 (of {m['n']})"
        if grazing.any():
            print(f"{what}: {int(grazing.sum())} values at N.V < {GRAZING_NV} miss R1, |e| up to {np.abs(m['e'][grazing]).max():.2f}")
        bad &= ~grazing
    if bad.any():
        idx = np.argwhere(bad)[:6]
        detail = [(tuple(int(v) for v in i), float(x[tuple(i)]), float(m["e"][tuple(i)])) for i in idx]
        raise AssertionError(f"{what}: R1 fails on {int(bad.sum())} of {m['n']} values, worst |e| {np.nanmax(np.abs(m['e'])):.2f} ulp; "
                             f"(index, exact, e): {detail}")
    assert m["misround"] <= r2_bound, f"{what}: R2 misrounding {m['misround']:.2e} > {r2_bound:.2e}"
    for key, n in (("mean", "n_rgb"), ("mean_low", "n_low"), ("mean_sky", "n_sky")):
        if m[n] >= R3_MIN_VALUES:
            assert abs(m[key]) <= 0.02, f"{what}: R3 {key} = {m[key]:+.4f} over {m[n]} values"
    print(f"{what}: max |e| {np.nanmax(np.abs(m['e'])):.3f}, misrounding {m['misround']:.2e}, mean e {m['mean']:+.4f} "
          f"(< 0.25: {m['mean_low']:+.4f} over {m['n_low']}, sky: {m['mean_sky']:+.4f} over {m['n_sky']})")
    return m


def _inputs(scene_name, mode, shadows, env_mip_count, w, h, seed, shipped=False, shadow_size=256):
    from unclerenderer_amd import hostmath, synth
    fc = hostmath.build_frame_constants(scene_name, w, h, shadow_size=shadow_size, shadow_strength=1.0 if shadows else 0.0,
                                        env_mip_count=env_mip_count)
    g = synth.gbuffer_scene(fc.view, fc.proj, fc.camera_position, w, h, seed) if mode == "scene" else synth.gbuffer_iid(w, h, seed)
    shadow = synth.shadow_map_noise(shadow_size, seed) if shadows else None
    if shipped:
        from pathlib import Path
        from unclerenderer_amd import assets
        adir = Path(__file__).parent / "golden" / "assets"
        env, base, mips, _ = assets.load_env_cube_dds(adir / "output_pmrem.dds")
        lut = assets.load_brdf_lut_dds(adir / "PreintegratedGF.dds")
    else:
        base, mips = 32, 6
        env, lut = synth.env_cube_procedural(base, mips), synth.brdf_lut_procedural(128, 32)
    return fc, g, shadow, env, base, mips, lut


def _tables(hotpath, shadow, env, base, mips, lut):
    from unclerenderer_amd.hotpath import to_device
    return hotpath.make_tables(to_device(shadow) if shadow is not None else None, hotpath.stage_env_cube(env, base, mips), base, mips,
                               to_device(lut))


def _launch(hotpath, form, stream, fc, g, tables, hdr_in, w, h):
    """One launch of `form` (lighting / sky / fused) on the kernel chosen by UR_OPT_LIGHTING_STREAM = stream; returns the bits."""
    from unclerenderer_amd import lib
    from unclerenderer_amd.hotpath import to_device
    torch = _torch()
    hotpath.set_option(lib.UR_OPT_LIGHTING_STREAM, stream)
    try:
        d = to_device(hdr_in)
        if form == "lighting":
            hotpath.deferred_lighting(fc.scene, to_device(g.A), to_device(g.B), to_device(g.C), tables, d, w, h)
        elif form == "sky":
            hotpath.sky_atmosphere(fc.sky, to_device(g.depth), d, w, h)
        else:
            hotpath.deferred_lighting_sky(fc.scene, fc.sky, to_device(g.A), to_device(g.B), to_device(g.C), to_device(g.depth), tables, d, w, h)
        torch.cuda.synchronize()
        return d.cpu().numpy().view(np.uint16)
    finally:
        hotpath.set_option(lib.UR_OPT_LIGHTING_STREAM, 1)


def _all_forms(hotpath, oracle, tag, fc, g, shadow, env, base, mips, lut, w, h, streams=(1, 0), forms=("lighting", "sky", "fused")):
    """Lighting only, sky only (over the oracle's lit frame) and the fused launch, on both kernels, against the restatement."""
    lit, frag = oracle.deferred_lighting(fc.scene, g.A, g.B, g.C, shadow, env, base, mips, lut, g.hdr, w, h, want_fragile=True)
    ref = oracle.sky_atmosphere(fc.sky, g.depth, lit, w, h)
    cube = r64.EnvCube(env, base, mips)
    xl, fl = r64.deferred_lighting64(fc.scene, g.A, g.B, g.C, shadow, env, base, mips, lut, g.hdr, w, h, env=cube)
    xs, fs = r64.sky_atmosphere64(fc.sky, g.depth, lit, w, h)       # sky over the oracle's lit bits: what the sky-only launch sees
    xf, ff = r64.sky_atmosphere64(fc.sky, g.depth, xl, w, h)        # lighting then sky, exact throughout
    sky = r64.sky_drawn(fc.sky, g.depth, w, h)
    nv = r64.n_dot_v(fc.scene, g.A, w, h)
    tables = _tables(hotpath, shadow, env, base, mips, lut) if forms != ("sky",) else None
    for stream in streams:
        for form in forms:
            what = f"{tag} {form} stream={stream}"
            if form == "lighting":
                check_accuracy(what, _launch(hotpath, form, stream, fc, g, tables, g.hdr, w, h), xl, fl, lit, frag, nv=nv)
            elif form == "sky":
                check_accuracy(what, _launch(hotpath, form, stream, fc, g, tables, lit, w, h), xs, fs, ref, None, sky)
            else:
                check_accuracy(what, _launch(hotpath, form, stream, fc, g, tables, g.hdr, w, h), xf, fl | ff, ref, frag, sky,
                               nv=np.where(sky, 1.0, nv))


@pytest.mark.parametrize("mode", ["scene", "iid"])
@pytest.mark.parametrize("scene_name", ["sponza", "duck"])
def test_lighting_and_sky_forms_are_faithful(hotpath, oracle, scene_name, mode):
    w, h = 320, 180
    fc, g, shadow, env, base, mips, lut = _inputs(scene_name, mode, True, 6, w, h, seed=11)
    _all_forms(hotpath, oracle, f"{scene_name}/{mode}", fc, g, shadow, env, base, mips, lut, w, h)


@pytest.mark.parametrize("shadows", [True, False])
@pytest.mark.parametrize("env_mip_count,irr_n", [(3, 8), (5, 2), (6, 1)])
def test_every_irradiance_table_form_is_faithful(hotpath, oracle, env_mip_count, irr_n, shadows):
    """The irradiance lookup at mip EnvMapMipCount - 1 of a 32^2 cube: faces of 8 texels are gathered from memory, faces of 2 and 1
    texels become per-cell polynomials in LDS."""
    w, h = 320, 180
    assert max(1, 32 >> (env_mip_count - 1)) == irr_n
    for mode in ("scene", "iid"):
        fc, g, shadow, env, base, mips, lut = _inputs("sponza", mode, shadows, env_mip_count, w, h, seed=41)
        _all_forms(hotpath, oracle, f"irr{irr_n}/{mode}/shadows={shadows}", fc, g, shadow, env, base, mips, lut, w, h, forms=("lighting", "fused"))


def test_shipped_ibl_assets_are_faithful(hotpath, oracle):
    w, h = 320, 180
    for mode in ("scene", "iid"):
        fc, g, shadow, env, base, mips, lut = _inputs("sponza", mode, True, 9, w, h, seed=77, shipped=True)
        _all_forms(hotpath, oracle, f"shipped/{mode}", fc, g, shadow, env, base, mips, lut, w, h, forms=("lighting", "fused"))


def test_view_ray_along_the_light_is_faithful(hotpath, oracle):
    """test_gpu_parity.py:test_lighting_view_ray_along_the_light's setup: V.L -> -1 around the frame's centre, lit, low roughness."""
    import dataclasses
    from unclerenderer_amd import hostmath, synth
    w, h = 320, 180
    base_preset = hostmath.SCENES["sponza"]
    L = hostmath.build_frame_constants(base_preset, w, h, shadow_size=256).light_direction.astype(np.float64)
    pos = np.array(base_preset.camera_position, np.float64)
    preset = dataclasses.replace(base_preset, camera_rotation_deg=None, camera_look_at=tuple(pos + 10.0 * L), light_intensity=3.0)
    fc = hostmath.build_frame_constants(preset, w, h, shadow_size=256, env_mip_count=6)
    P = np.asarray(fc.proj, np.float32).reshape(4, 4)
    xs, ys = np.meshgrid(np.arange(w, dtype=np.float64) + 0.5, np.arange(h, dtype=np.float64) + 0.5)
    a, b = (xs / w * 2 - 1) / P[0, 0], -(ys / h * 2 - 1) / P[1, 1]
    r = np.maximum(np.sqrt(a * a + b * b), 1e-9)
    t2 = np.stack([-a / r, -b / r, np.zeros_like(r)], -1)
    t1 = np.stack([b / r, -a / r, np.zeros_like(r)], -1)
    N = 0.7 * t1 + 0.7 * t2 + (0.3 * 0.7 * r)[..., None] * np.array([0.0, 0.0, 1.0])
    N /= np.linalg.norm(N, axis=-1, keepdims=True)
    A = np.concatenate([N, np.full((h, w, 1), -5.0)], -1).astype(np.float16).view(np.uint16)
    rough = 0.08 + 0.2 * synth.hash_unit(77, *synth._grid(w, 0, h), 0)
    B = np.stack([np.full((h, w), 0.04), np.zeros((h, w)), rough, np.ones((h, w))], -1).astype(np.float16).view(np.uint16)
    Cc = np.full((h, w), 0xFF909090, np.uint32)
    hdr = np.zeros((h, w, 4), np.float16)
    hdr[..., 3] = 1.0
    g = synth.GBuffer(w, h, 0, h, A, B, Cc, hdr.view(np.uint16), np.full((h, w), fc.near / 5.0, np.float32))
    shadow = np.ones((256, 256), np.float32)
    env, lut = synth.env_cube_procedural(32, 6), synth.brdf_lut_procedural(128, 32)
    _all_forms(hotpath, oracle, "into-the-light", fc, g, shadow, env, 32, 6, lut, w, h, forms=("lighting",))


def test_c2_1080p_in_full_is_faithful(hotpath, oracle):
    """C2 (Sponza 1920x1080, shipped IBL tables, a 2048^2 scene shadow map), fused, every pixel."""
    from unclerenderer_amd import hostmath, synth
    w, h = 1920, 1080
    fc = hostmath.build_frame_constants("sponza", w, h, shadow_size=2048, env_mip_count=9)
    g = synth.gbuffer_scene(fc.view, fc.proj, fc.camera_position, w, h, synth.SEED_BASE + 2)
    shadow = synth.shadow_map_scene(np.ctypeslib.as_array(fc.scene.LightViewProjection), 2048)
    _, _, _, env, base, mips, lut = _inputs("sponza", "iid", False, 9, 8, 8, seed=0, shipped=True)
    oracle.set_threads(oracle.hardware_threads())
    try:
        _all_forms(hotpath, oracle, "C2", fc, g, shadow, env, base, mips, lut, w, h, streams=(1,), forms=("fused",))
    finally:
        oracle.set_threads(1)


@pytest.mark.parametrize("w,h,mode", [(3840, 2160, "scene"), (7680, 4320, "iid")])
def test_4k_8k_sample_is_faithful(hotpath, oracle, w, h, mode):
    """The whole frame shaded in one fused launch. Checked against the oracle and the restatement on 30 random full rows plus two
    full rows across a 4-row tile boundary (the frame's middle); against the restatement alone on ~2e5 random pixels and two full
    columns across a 16-column tile boundary (a quarter of the width), R2 scaled by the oracle's misrounding on the rows."""
    from unclerenderer_amd import hostmath, synth
    fc = hostmath.build_frame_constants("sponza", w, h, shadow_size=2048, env_mip_count=9)
    g = synth.gbuffer_scene(fc.view, fc.proj, fc.camera_position, w, h, 5) if mode == "scene" else synth.gbuffer_iid(w, h, 5)
    shadow = synth.shadow_map_noise(2048, 5)
    _, _, _, env, base, mips, lut = _inputs("sponza", "iid", False, 9, 8, 8, seed=0, shipped=True)
    tables = _tables(hotpath, shadow, env, base, mips, lut)
    out = _launch(hotpath, "fused", 1, fc, g, tables, g.hdr, w, h)
    cube = r64.EnvCube(env, base, mips)
    rng = np.random.default_rng(w + h)
    r0, c0 = h // 2 - 1, w // 4 - 1
    rows = sorted(set(rng.choice(h, 30, replace=False).tolist()) | {r0, r0 + 1})
    refs, frags, xs_, f64s = [], [], [], []
    for r in rows:
        sl = slice(r, r + 1)
        lit, frag = oracle.deferred_lighting(fc.scene, g.A[sl], g.B[sl], g.C[sl], shadow, env, base, mips, lut, g.hdr[sl], w, h, r, 1,
                                             want_fragile=True)
        ref = oracle.sky_atmosphere(fc.sky, g.depth[sl], lit, w, h, r, 1)
        nbad, worst, _ = hdr_mismatch(out[sl], ref, exclude=frag)
        assert nbad == 0, f"row {r}: {nbad} channel values beyond max(1e-3, 1 ulp) of the oracle (worst excess {worst})"
        x, f64 = r64.lighting_sky64(fc.scene, fc.sky, g.A[sl], g.B[sl], g.C[sl], g.depth[sl], shadow, env, base, mips, lut, g.hdr[sl], w, h,
                                    r, 1, env=cube)
        refs.append(ref), frags.append(np.asarray(frag, bool)), xs_.append(x), f64s.append(f64)
    sky_rows = np.concatenate([r64.sky_drawn(fc.sky, g.depth[r:r + 1], w, h, r, 1) for r in rows])
    nv_rows = np.concatenate([r64.n_dot_v(fc.scene, g.A[r:r + 1], w, h, r, 1) for r in rows])
    frag_rows, f64_rows = np.concatenate(frags), np.concatenate(f64s)
    ref_rows, x_rows = np.concatenate(refs), np.concatenate(xs_)
    check_accuracy(f"{w}x{h} {len(rows)} rows", out[rows], x_rows, f64_rows, ref_rows, frag_rows, sky_rows, nv=np.where(sky_rows, 1.0, nv_rows))
    oracle_misround = r64.measure(ref_rows, x_rows, frag_rows | f64_rows)["misround"]

    n = 200_000
    ys = np.concatenate([rng.integers(0, h, n), np.arange(h), np.arange(h)])
    xs = np.concatenate([rng.integers(0, w, n), np.full(h, c0), np.full(h, c0 + 1)])
    x, f64 = r64.lighting_sky64(fc.scene, fc.sky, g.A, g.B, g.C, g.depth, shadow, env, base, mips, lut, g.hdr, w, h, pixels=(ys, xs), env=cube)
    sky = r64.sky_drawn(fc.sky, g.depth, w, h, pixels=(ys, xs))
    nv = np.where(sky, 1.0, r64.n_dot_v(fc.scene, g.A, w, h, pixels=(ys, xs)))
    check_accuracy(f"{w}x{h} sample", out[ys, xs], x, f64, sky=sky, oracle_misround=oracle_misround, nv=nv)
