"""The float64 restatement of DeferredLighting / SkyAtmosphere (tests/lighting_ref64.py): hand-derived known answers, and the
fp32 oracle measured against it. Outside the pixels whose discontinuous decisions sit on a threshold, every oracle value must
be within one fp16 ulp of the exact value (rule R1 of tests/test_gpu_accuracy.py with the oracle in the kernel's place); its
misrounding rate and mean signed error are the fp32 yardstick the GPU rules are scaled by."""
import math
from pathlib import Path

import numpy as np
import pytest

from tests import lighting_ref64 as r64
from unclerenderer_amd import hostmath, lib, synth

ADIR = Path(__file__).parent / "golden" / "assets"


# ---------------------------------------------------------------------------------------------------------------------
# known answers: 1x1 frames looking down the view axis, a constant environment and a constant LUT
# ---------------------------------------------------------------------------------------------------------------------
E = np.array([0.25, 0.5, 1.0])
LA, LB = 32768 / 65535, 16384 / 65535


def _const_cube(base, mips, color):
    out = []
    for _ in range(6):
        for m in range(mips):
            n = max(1, base >> m)
            t = np.zeros((n * n, 4), np.float16)
            t[:, :3] = color
            t[:, 3] = 1
            out.append(t.view(np.uint16))
    return np.concatenate(out)


def _pixel_case(urlib, normal, smr, rgb, light_intensity=2.0, light_color=(1.0, 0.5, 0.25), light_dir=(0.0, 0.0, -1.0), view_z=4.0):
    """One pixel whose view ray is (0, 0, 1) at view depth view_z (V = (0, 0, -1)); identity view; the camera at the origin."""
    import ctypes as C
    view = np.eye(4, dtype=np.float32).ravel()
    proj = hostmath.reverse_z_projection(math.radians(90), 1.0, 0.1)
    sc = lib.SceneConstants()
    urlib.ur_host_fill_scene_constants(lib.fptr(view), lib.fptr(proj), lib.fptr(np.zeros(3, np.float32)), light_intensity,
                                       lib.fptr(np.array(light_dir, np.float32)), lib.fptr(np.array(light_color, np.float32)),
                                       lib.fptr(np.eye(4, dtype=np.float32).ravel()), 0.0, 0.0, 0.0, 0.0, 3.0, C.byref(sc))
    cube = _const_cube(4, 3, E)
    lut = np.zeros((4, 4, 2), np.uint16)
    lut[..., 0], lut[..., 1] = 32768, 16384
    A = np.array([[[*normal, -view_z]]], np.float16).view(np.uint16)
    B = np.array([[[*smr, 1.0]]], np.float16).view(np.uint16)
    Cc = np.array([[rgb[0] | (rgb[1] << 8) | (rgb[2] << 16) | (255 << 24)]], np.uint32)
    hdr = np.array([[[0.5, 0.0, 0.0, 1.0]]], np.float16).view(np.uint16)
    x, frag = r64.deferred_lighting64(sc, A, B, Cc, None, cube, 4, 3, lut, hdr, 1, 1)
    assert not frag.any()
    n16 = np.array(normal, np.float16).astype(np.float64)
    smr16 = np.array(smr, np.float16).astype(np.float64)
    alb = np.array([((c / 255 + 0.055) / 1.055) ** 2.4 if c / 255 > 0.04045 else c / 255 / 12.92 for c in rgb])
    return x[0, 0], n16 / np.linalg.norm(n16), smr16, alb, np.array(light_color) * light_intensity


def _ggx_pixel(n, smr, alb, light, L):
    """PBRCommon.hlsl's EvaluatePBR by hand for V = (0, 0, -1): returns the direct term."""
    V = np.array([0.0, 0.0, -1.0])
    f0s, m, r = smr
    F0 = f0s + (alb - f0s) * m
    Hh = (V + L) / np.linalg.norm(V + L)
    nl, nv, nh, vh = (min(max(float(np.dot(a, b)), 0.0), 1.0) for a, b in ((n, L), (n, V), (n, Hh), (V, Hh)))
    a2 = (r * r) ** 2
    D = a2 / max(math.pi * ((nh * nh) * (a2 - 1) + 1) ** 2, 1e-4)
    k = (r + 1) ** 2 / 8
    G = nv / (nv * (1 - k) + k) * nl / (nl * (1 - k) + k)
    F = F0 + (1 - F0) * (1 - vh) ** 5
    return ((1 - F) * (1 - m) * alb + D * G * F / max(4 * nl * nv, 1e-4)) * nl * light


def _ambient(smr, alb):
    f0s, m, _ = smr
    F0 = f0s + (alb - f0s) * m
    return E * alb * (1 - m) + E * (F0 * LA + LB)


def test_lighting_pixel_analytic_known_answer(urlib):
    """test_oracle_kat.py:test_lighting_pixel_analytic: N = V = L, dielectric, roughness 1: D = 1/pi, G = 1, F = F0."""
    x, n, smr, alb, light = _pixel_case(urlib, (0.0, 0.0, -1.0), (0.04, 0.0, 1.0), (188, 188, 188))
    f0 = smr[0]
    want = np.array([0.5, 0, 0]) + ((1 - f0) * alb + f0 / (4 * math.pi)) * light + E * alb + E * (f0 * LA + LB)
    np.testing.assert_allclose(x[:3], want, rtol=1e-6)
    assert x[3] == 2.0


def test_grazing_pixel_known_answer(urlib):
    """N.V = N.L = 1.7e-3 (N almost perpendicular to the view ray, L = V): 4 N.L N.V = 1.2e-5 sits under the 1e-4 clamp."""
    th = math.radians(89.9)
    x, n, smr, alb, light = _pixel_case(urlib, (math.sin(th), 0.0, -math.cos(th)), (0.04, 0.0, 0.5), (200, 120, 40))
    nv = float(-n[2])
    assert 0 < 4 * nv * nv < 1e-4
    f0, r = smr[0], smr[2]
    a2 = r ** 4
    D = a2 / (math.pi * ((nv * nv) * (a2 - 1) + 1) ** 2)
    k = (r + 1) ** 2 / 8
    G = (nv / (nv * (1 - k) + k)) ** 2
    direct = ((1 - f0) * alb + D * G * f0 / 1e-4) * nv * light  # V = H: F = F0
    want = np.array([0.5, 0, 0]) + direct + _ambient(smr, alb)
    np.testing.assert_allclose(x[:3], want, rtol=1e-6)
    np.testing.assert_allclose(direct, _ggx_pixel(n, smr, alb, light, np.array([0.0, 0.0, -1.0])), rtol=1e-12)


@pytest.mark.parametrize("rough", [0.0, 1.0])
def test_roughness_extremes_known_answer(urlib, rough):
    """Light 60 degrees off the view ray, N halfway between: roughness 0 gives alpha = 0 so D = 0 (no specular at all);
    roughness 1 gives D = 1/pi whatever N.H is."""
    L = np.array([math.sin(math.radians(60)), 0.0, -math.cos(math.radians(60))])
    Hh = (L + np.array([0.0, 0.0, -1.0]))
    Hh /= np.linalg.norm(Hh)
    x, n, smr, alb, light = _pixel_case(urlib, tuple(Hh), (0.04, 0.0, rough), (90, 160, 230), light_dir=tuple(L))
    nl, nv = float(np.dot(n, L)), float(-n[2])
    vh = math.cos(math.radians(30))
    f0 = smr[0]
    F = f0 + (1 - f0) * (1 - vh) ** 5
    if rough == 0.0:
        spec = 0.0
    else:
        k = 0.5
        G = nv / (nv * (1 - k) + k) * nl / (nl * (1 - k) + k)
        spec = (1 / math.pi) * G * F / (4 * nl * nv)
    direct = ((1 - F) * alb + spec) * nl * light
    want = np.array([0.5, 0, 0]) + direct + _ambient(smr, alb)
    np.testing.assert_allclose(x[:3], want, rtol=1e-6)


def test_metallic_pixel_known_answer(urlib):
    """Metallic 1, N = V = L, roughness 1: F0 = albedo, no diffuse (direct or ambient): direct = albedo / (4 pi)."""
    x, n, smr, alb, light = _pixel_case(urlib, (0.0, 0.0, -1.0), (0.04, 1.0, 1.0), (188, 90, 30))
    want = np.array([0.5, 0, 0]) + alb / (4 * math.pi) * light + E * (alb * LA + LB)
    np.testing.assert_allclose(x[:3], want, rtol=1e-6)


def _sky_1x1(view_rows, light_dir, cam_y=0.0):
    s = lib.SkyConstants()
    v = np.eye(4)
    v[:3, :3] = view_rows
    s.View[:] = v.ravel().astype(np.float32)
    p = np.zeros(16, np.float32)
    p[0] = p[5] = 1.0
    p[11], p[14] = 1.0, 0.1
    s.Projection[:] = p
    w = np.eye(4, dtype=np.float32) * 500.0
    w[3, 3] = 1.0
    s.World[:] = w.ravel()
    s.LightDirection[:] = light_dir
    s.LightColor[:] = (1.0, 0.95, 0.9)
    s.CameraPosition[:] = (0.0, cam_y, 0.0)
    return s


def _atmosphere_by_hand(view_y, cos_sun_view, cos_sun_up, color, cam_y):
    falloff = (1 - (view_y * 0.5 + 0.5)) ** 3
    base = np.array([0.05, 0.12, 0.22]) + falloff * (np.array([0.52, 0.68, 0.86]) - np.array([0.05, 0.12, 0.22]))
    ray = 3.0 / (16.0 * math.pi) * (1 + cos_sun_view ** 2)
    g = 0.76
    mie = (1 - g * g) / (4 * math.pi * max((1 + g * g - 2 * g * cos_sun_view) ** 1.5, 1e-3))
    scat = np.array([0.65, 0.57, 0.475]) * math.exp(-cam_y / 8000) * ray + np.array(color) * math.exp(-cam_y / 1200) * mie * 0.8
    return base + scat * math.exp(-max(0.0, 1 - cos_sun_up) * 2)


@pytest.mark.parametrize("case", ["sun", "zenith"])
def test_sky_rays_known_answers(case):
    """The centre ray of a 1x1 frame: towards the sun (cos = 1: Mie's forward peak, (1 - g^2) / (4 pi (1 - g)^3)) with the sun 37
    degrees up, and straight up (falloff 0: the zenith colour) with the camera 1200 m high."""
    if case == "sun":
        rows, light, cam_y, view_y, csv, csu = [[1, 0, 0], [0, 0.8, 0.6], [0, -0.6, 0.8]], (0.0, 0.6, 0.8), 0.0, 0.6, 1.0, 0.6
    else:
        rows, light, cam_y, view_y, csv, csu = [[1, 0, 0], [0, 0, 1], [0, -1, 0]], (0.0, 0.6, 0.8), 1200.0, 1.0, 0.6, 0.6
    sky = _sky_1x1(np.array(rows, np.float64), light, cam_y)
    depth = np.zeros((1, 1), np.float32)
    hdr = np.zeros((1, 1, 4), np.uint16)
    x, frag = r64.sky_atmosphere64(sky, depth, hdr, 1, 1)
    assert not frag.any() and r64.sky_drawn(sky, depth, 1, 1).all()
    want = _atmosphere_by_hand(view_y, csv, csu, (1.0, 0.95, 0.9), cam_y)
    np.testing.assert_allclose(x[0, 0, :3], want, rtol=1e-6)
    assert x[0, 0, 3] == 1.0
    # the sphere's depth along the ray is near / radius: a stored depth just above it is not overwritten
    _, f2 = r64.sky_atmosphere64(sky, np.full((1, 1), 0.1 / 500.0, np.float32), hdr, 1, 1)
    assert f2.all()
    assert not r64.sky_drawn(sky, np.full((1, 1), 0.1 / 500.0 * 1.001, np.float32), 1, 1).any()


def test_cleared_pixels_shade_to_nan(urlib):
    with np.errstate(invalid="ignore"):
        x, *_ = _pixel_case(urlib, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0, 0, 0))
    assert np.isnan(x[:3]).all() and x[3] == 2.0


def test_cube_fold_matches_the_bordered_staging(oracle):
    """The fold tables are the seamless-edge rule: every bordered texel the oracle stages (uro_stage_env_cube) is the texel the
    fold table names, for face sizes 8, 4, 2 and 1."""
    env = synth.env_cube_procedural(8, 4)
    staged = oracle.stage_env_cube(env, 8, 4).view(np.float16).astype(np.float64)[:, :3]
    cube = r64.EnvCube(env, 8, 4)
    off = 0
    for m, n in enumerate(cube.sizes):
        e = (n + 2) ** 2
        for f in range(6):
            want = staged[off:off + e].reshape(n + 2, n + 2, 3)
            np.testing.assert_array_equal(cube.texels[cube.fold[m][f]], want, err_msg=f"mip {m} face {f}")
            off += e


# ---------------------------------------------------------------------------------------------------------------------
# the oracle is a faithful fp32 evaluation of the restatement
# ---------------------------------------------------------------------------------------------------------------------
W, H = 320, 180
# (scene preset, G-buffer, shadows, env mips of a 32^2 procedural cube or "shipped" for output_pmrem.dds + PreintegratedGF.dds)
FIXTURES = [("sponza", "scene", True, 5), ("sponza", "iid", True, 5), ("duck", "scene", True, 5), ("duck", "iid", True, 5),
            ("sponza", "scene", False, 6), ("duck", "iid", False, 3), ("sponza", "iid", True, 3), ("duck", "scene", True, 6),
            ("sponza", "scene", True, "shipped"), ("sponza", "iid", True, "shipped")]
# The fp32 yardstick as measured on these fixtures: the oracle's misrounding rate (values != round16(x)) and mean signed error
# over RGB, outside fragile | fragile64, after lighting + sky. A correctly rounded fp32 evaluation misrounds only values whose
# exact value lies within ~1e-3 ulp of a rounding boundary.
YARDSTICK = {
    ("sponza", "scene", True, 5): (2.7e-4, -3e-5), ("sponza", "iid", True, 5): (1.6e-4, -2.9e-4),
    ("duck", "scene", True, 5): (2.6e-4, -3.8e-4), ("duck", "iid", True, 5): (1.5e-4, +4.7e-5),
    ("sponza", "scene", False, 6): (6.9e-5, -1.7e-3), ("duck", "iid", False, 3): (1.8e-4, -2.9e-4),
    ("sponza", "iid", True, 3): (2.1e-4, -6.0e-4), ("duck", "scene", True, 6): (2.6e-4, +1.4e-4),
    ("sponza", "scene", True, "shipped"): (5.2e-4, +2.1e-5), ("sponza", "iid", True, "shipped"): (2.9e-4, -1.1e-3),
}


def fixture_inputs(scene_name, mode, shadows, mips, w=W, h=H, seed=11):
    """Inputs of one fixture: (fc, g, shadow or None, env, base, mips, lut)."""
    if mips == "shipped":
        from unclerenderer_amd import assets
        env, base, mips, _ = assets.load_env_cube_dds(ADIR / "output_pmrem.dds")
        lut = assets.load_brdf_lut_dds(ADIR / "PreintegratedGF.dds")
    else:
        base, env, lut = 32, synth.env_cube_procedural(32, mips), synth.brdf_lut_procedural(128, 32)
    fc = hostmath.build_frame_constants(scene_name, w, h, shadow_size=256, shadow_strength=1.0 if shadows else 0.0, env_mip_count=mips)
    g = synth.gbuffer_scene(fc.view, fc.proj, fc.camera_position, w, h, seed) if mode == "scene" else synth.gbuffer_iid(w, h, seed)
    shadow = synth.shadow_map_noise(256, seed) if shadows else None
    return fc, g, shadow, env, base, mips, lut


@pytest.mark.parametrize("fx", FIXTURES, ids=lambda f: "-".join(map(str, f)))
def test_oracle_is_faithful_to_the_restatement(oracle, urlib, fx, record_property):
    fc, g, shadow, env, base, mips, lut = fixture_inputs(*fx)
    lit, frag = oracle.deferred_lighting(fc.scene, g.A, g.B, g.C, shadow, env, base, mips, lut, g.hdr, W, H, want_fragile=True)
    ref = oracle.sky_atmosphere(fc.sky, g.depth, lit, W, H)
    cube = r64.EnvCube(env, base, mips)
    xl, fl = r64.deferred_lighting64(fc.scene, g.A, g.B, g.C, shadow, env, base, mips, lut, g.hdr, W, H, env=cube)
    xs, fs = r64.sky_atmosphere64(fc.sky, g.depth, xl, W, H)
    sky = r64.sky_drawn(fc.sky, g.depth, W, H)
    assert frag.mean() < 5e-3 and (fl | fs).mean() < 5e-3
    for name, bits, x, f64 in (("lighting", lit, xl, fl), ("lighting+sky", ref, xs, fl | fs)):
        skip = frag.astype(bool) | f64
        m = r64.measure(bits, x, skip, sky if name == "lighting+sky" else None)
        assert m["nan_mismatch"] == 0, f"{name}: NaN positions differ from the restatement's on {m['nan_mismatch']} values"
        bad = r64.r1_violations(m["e"])
        assert not bad.any(), (f"{name}: {int(bad.sum())} oracle values more than one ulp from the exact value, worst "
                               f"{np.nanmax(np.abs(m['e'])):.2f} ulp at {np.argwhere(bad)[:4].tolist()}")
        assert m["n"] > 0.9 * W * H * 4
        record_property(f"{name} misround", m["misround"])
        record_property(f"{name} mean_e", m["mean"])
        print(f"{fx} {name}: oracle misrounding {m['misround']:.2e}, mean e {m['mean']:+.2e} (below 0.25: {m['mean_low']:+.2e}, "
              f"sky: {m['mean_sky']:+.2e}), max |e| {np.nanmax(np.abs(m['e'])):.3f}")
    rate, bias = YARDSTICK[fx]
    assert m["misround"] <= 1.5 * rate + 5e-5, f"misrounding {m['misround']:.2e} against the recorded {rate:.1e}"
    assert abs(m["mean"] - bias) <= 5e-4, f"mean e {m['mean']:+.2e} against the recorded {bias:+.1e}"
    assert abs(m["mean_low"]) <= 5e-3 and abs(m["mean_sky"]) <= 5e-3
    if fx[1] == "iid":
        assert np.isnan(x[g.depth == 0][:, :3]).sum() == 0 and np.isnan(xl[g.depth == 0][:, :3]).all()


def test_pixel_sample_equals_the_whole_frame(oracle, urlib):
    """The pixel-list form evaluates exactly what the whole-frame form does at those pixels, on a band."""
    fc, g, shadow, env, base, mips, lut = fixture_inputs("sponza", "scene", True, 5)
    r0, rows = 37, 61
    sl = slice(r0, r0 + rows)
    args = (fc.scene, fc.sky, g.A[sl], g.B[sl], g.C[sl], g.depth[sl], shadow, env, base, mips, lut, g.hdr[sl], W, H, r0, rows)
    x, f = r64.lighting_sky64(*args)
    rng = np.random.default_rng(3)
    ys, xs = rng.integers(0, rows, 500), rng.integers(0, W, 500)
    xp, fp = r64.lighting_sky64(*args, pixels=(ys, xs))
    np.testing.assert_array_equal(xp, x[ys, xs])
    np.testing.assert_array_equal(fp, f[ys, xs])


# ---------------------------------------------------------------------------------------------------------------------
# the rules have teeth: errors of the size the old 1e-3 floor admitted fail R1 or R3
# ---------------------------------------------------------------------------------------------------------------------
def _planted(bits, fn):
    v = bits.view(np.float16).astype(np.float64)
    out = v.copy()
    out[..., :3] = fn(v[..., :3])
    return out.astype(np.float16).view(np.uint16)


@pytest.mark.parametrize("mode", ["scene", "iid"])
def test_small_systematic_errors_fail_the_rules(oracle, urlib, mode):
    from tests.util import hdr_mismatch
    fc, g, shadow, env, base, mips, lut = fixture_inputs("sponza", mode, True, 5)
    lit, frag = oracle.deferred_lighting(fc.scene, g.A, g.B, g.C, shadow, env, base, mips, lut, g.hdr, W, H, want_fragile=True)
    ref = oracle.sky_atmosphere(fc.sky, g.depth, lit, W, H)
    x, f64 = r64.lighting_sky64(fc.scene, fc.sky, g.A, g.B, g.C, g.depth, shadow, env, base, mips, lut, g.hdr, W, H)
    skip = frag.astype(bool) | f64
    e_ref = r64.measure(ref, x, skip)["e"]
    ulp = lambda v: r64.ulp16(v)
    plants = {"+4e-4": lambda v: v + 4e-4, "x1.0035 below 0.25": lambda v: np.where(v < 0.25, v * 1.0035, v),
              "+3 ulp below 0.5": lambda v: np.where(v < 0.5, v + 3 * ulp(v), v)}
    for name, fn in plants.items():
        bad = _planted(ref, fn)
        assert hdr_mismatch(bad, ref, exclude=frag)[0] == 0, f"{name}: the 1e-3 floor alone should admit this error"
        m = r64.measure(bad, x, skip)
        r1 = int(r64.r1_violations(m["e"], e_ref).sum())
        r3 = abs(m["mean"]) > 0.02 or abs(m["mean_low"]) > 0.02
        assert r1 > 0 or r3, name
