"""The ray caster's textured, masked and forward pieces (tests/raycast_tex.py) against hand-worked answers, its left-out share under the
cap on every new scene, the restatements gbuffer_tex_ref.gbuffer_pass, gbuffer_mask_ref.masked_pass and forward_ref.forward_pass held to
it on connected meshes under real cameras, and nine planted errors that show the comparison bites. The GPU files assert that the kernels
equal the restatements byte for byte, so this file holds the kernels transitively; tests/test_gpu_raycast_tex.py holds them directly."""
import copy

import numpy as np
import pytest

from tests import depth_ref as D
from tests import forward_ref as FW
from tests import gbuffer_mask_ref as M
from tests import gbuffer_tex_ref as X
from tests import raycast_ref as R
from tests import raycast_tex as T
from tests.test_raycast_ref import HAND_PROJ, IDENTITY, NEAR, report

pytestmark = pytest.mark.usefixtures("urlib")  # the scenes' cameras come from the library's host math

W0, H0 = R.TARGETS[0]
F = np.float32


# ---- hand-worked answers: a plane z = const that fills the 8 x 8 view (clip = (x, y, NEAR, z)) ----------------------------------------------

def _plane(z, uv=None, vertex_alpha=None, tangent=(1, 0, 0, 1), cls=X.TexDraw, **kw):
    """The facing triangle of tests/test_raycast_ref.py at depth z. The texel centre (px + 0.5, py + 0.5) meets it at x = z ((px + 0.5) / 4
    - 1), y = z (1 - (py + 0.5) / 4); by default TEXCOORD is ((x + z) / 2z, (z - y) / 2z) = ((px + 0.5) / 8, (py + 0.5) / 8) there."""
    p = np.array([(-20, -10, z), (20, -10, z), (0, 30, z)], np.float64)
    v = np.zeros((3, 16), F)
    v[:, 0:3], v[:, 3:6], v[:, 8:12], v[:, 12:16] = p, (0, 0, -1), tangent, 1.0
    t = np.stack([(p[:, 0] + z) / (2 * z), (z - p[:, 1]) / (2 * z)], axis=1)
    v[:, 6:8] = t if uv is None else uv(t)
    if vertex_alpha is not None:
        v[:, 15] = vertex_alpha(t)
    return cls(v.reshape(-1).view(np.uint8).copy(), np.arange(3, dtype=np.uint32), **kw)


RAMP8 = T.Analytic("ramp", a=(10, 20, 30, 255), bx=(2, 4, 0, 0), by=(16, 0, 6, 0), size=8, mips=1)  # texel (i, j) holds a + bx i + by j
PX, PY = np.meshgrid(np.arange(8), np.arange(8))


def _code(i, j):
    return (np.array(RAMP8.a[:3]) + i[..., None] * np.array(RAMP8.bx[:3]) + j[..., None] * np.array(RAMP8.by[:3])) / 255.0


def test_uv_at_a_known_texel():
    d = _plane(2.0, emissive=np.array([1.0, 2.0, 0.5], F))
    rc = T.cast([d], 8, 8, IDENTITY, HAND_PROJ, [{"key": 8, "emissive": RAMP8}])
    assert rc["hit"].all() and np.allclose(rc["emissive"][0], [1.0, 2.0, 0.5] * _code(PX, PY), rtol=0, atol=1e-13)
    assert np.allclose(rc["albedo"], 1.0) and np.allclose(rc["metallic"], 0.0) and np.allclose(rc["roughness"], 1.0)  # the other bits are clear


def test_rotated_transform():
    """Rotation (cos, sin) = (0, 1) and offset (1, 0): (u, v) -> (u 0 - v 1 + 1, u 1 + v 0) = (1 - v, u), so texel (px, py) of the target
    shows texel (7 - py, px) of the map. A negated sine would give (1 + v, -u): another texel."""
    d = _plane(2.0, emissive=np.ones(3, F), transforms={"emissive": ((1.0, 0.0), (1.0, 1.0), (0.0, 1.0))})
    rc = T.cast([d], 8, 8, IDENTITY, HAND_PROJ, [{"key": 8, "emissive": RAMP8}])
    assert np.allclose(rc["emissive"][0], _code(7 - PY, PX), rtol=0, atol=1e-13)


def test_tangent_frame_with_negative_w():
    """n = (0, 0, -1), t = (1, 0, 0): cross(n, t) = (0, -1, 0), times w = -1 the bitangent (0, 1, 0). The map's codes (204, 51, 0) give
    r, g = (0.6, -0.6): the base pass reconstructs z = sqrt(0.28) and gets 0.6 t - 0.6 b + z n = (0.6, -0.6, -sqrt(0.28)), the forward pass
    takes b = -1 and gets (0.6, -0.6, 1) / sqrt(1.72). With w = +1 the y component is +0.6."""
    mats = [{"key": 1, "normal": T.Analytic("const", a=(204, 51, 0, 255))}]
    rc = T.cast([_plane(2.0, tangent=(1, 0, 0, -1))], 8, 8, IDENTITY, HAND_PROJ, mats)
    assert np.allclose(rc["normal"], [0.6, -0.6, -np.sqrt(0.28)], rtol=0, atol=1e-13)
    assert np.allclose(rc["fnormal"], np.array([0.6, -0.6, 1.0]) / np.sqrt(1.72), rtol=0, atol=1e-13)
    rc = T.cast([_plane(2.0, tangent=(1, 0, 0, 1))], 8, 8, IDENTITY, HAND_PROJ, mats)
    assert np.allclose(rc["normal"], [0.6, 0.6, -np.sqrt(0.28)], rtol=0, atol=1e-13)


def test_alpha_band_ends_at_a_known_column():
    """COLOR.a = u = (px + 0.5) / 8 under BaseColorAlpha 1 and a cutoff of 0.5: columns 0-3 (alpha up to 0.4375) are discarded and show
    the opaque plane at z = 4 behind one discarded hit, columns 4-7 (from 0.5625) keep the masked plane at z = 2."""
    draws = [_plane(4.0, cls=M.MaskDraw), _plane(2.0, vertex_alpha=lambda t: t[:, 0], cls=M.MaskDraw, cutoff=0.5)]
    rc = T.cast(draws, 8, 8, IDENTITY, HAND_PROJ, [{"key": 0}, {"key": M.ALPHA_MASK}], masked=(1,))
    assert rc["hit"].all() and (rc["draw"][:, :, :4] == 0).all() and (rc["draw"][:, :, 4:] == 1).all()
    assert (rc["discards"][:, :, :4] == 1).all() and (rc["discards"][:, :, 4:] == 0).all()
    assert np.allclose(rc["depth"][:, :, :4], NEAR / 4, rtol=0, atol=1e-15) and np.allclose(rc["depth"][:, :, 4:], NEAR / 2, rtol=0, atol=1e-15)
    assert np.allclose(rc["alpha_margin"][0, :, :, 0], (PX + 0.5) / 8 - 0.5, rtol=0, atol=1e-13)
    compared, any_hit, share = T.classify(rc)
    assert compared.all() and any_hit.all() and share == 0.0
    # without the material's bit, or outside the masked selection, nothing is discarded
    for mats, masked in (([{"key": 0}, {"key": 0}], (1,)), ([{"key": 0}, {"key": M.ALPHA_MASK}], ())):
        assert (T.cast(draws, 8, 8, IDENTITY, HAND_PROJ, mats, masked=masked)["draw"] == 1).all()


def test_level_is_exactly_one_at_two_to_one_minification():
    """TEXCOORD (0.275 u, 0.5 v) of the default: a pixel spans 0.275 x 64 / 8 = 2.2 texels of the 64-texel map across and 4 down, so
    N = ceil(4 / 2.2) = 2 and each probe minifies 2 : 1: level = log2(4 / 2) = 1, and the level-coded map returns 60 / 255. (An exactly
    isotropic footprint would leave N = 1 or 2 to the last bit of the ratio.)"""
    d = _plane(2.0, uv=lambda t: t * [0.275, 0.5], emissive=np.ones(3, F))
    rc = T.cast([d], 8, 8, IDENTITY, HAND_PROJ, [{"key": 8, "emissive": T.LEVELS}])
    assert (rc["N_emissive"] == 2).all() and not rc["n_disagree"].any()
    assert np.allclose(rc["level_emissive"], 1.0, rtol=0, atol=1e-12) and np.allclose(rc["level_tol_emissive"], 0.0, rtol=0, atol=1e-12)
    assert np.allclose(rc["emissive"], 60.0 / 255.0, rtol=0, atol=1e-13)


def test_analytic_textures_hold_what_they_promise():
    for a in list(T.RAMPS.values()) + [T.MASK_BASE]:
        tex = a.tex()
        assert [lv.shape for lv in tex.levels] == [(64, 64, 4), (32, 32, 4), (16, 16, 4), (8, 8, 4)] and not tex.srgb
        u = v = np.array([(10 + 0.5) / 64])  # the centre of texel (10, 10) of level 0
        assert np.allclose(a.value(u, v)[0], tex.levels[0][10, 10] / 255.0, rtol=0, atol=1e-15)
        u = v = np.array([(2 + 0.5) / 16])   # ... and of texel (2, 2) of level 2: the same affine function
        assert np.allclose(a.value(u, v)[0], tex.levels[2][2, 2] / 255.0, rtol=0, atol=1e-15)
    assert [int(lv[0, 0, 0]) for lv in T.LEVELS.tex().levels] == [0, 60, 120, 180]
    with pytest.raises(AssertionError):
        T.Analytic("ramp", a=(0, 0, 0, 0), bx=(1, 0, 0, 0)).tex()  # an odd slope: half codes at level 1
    # the restatement's own sampler in float64 returns the ramp's function whatever N and L are, clear of the seam
    rng = np.random.default_rng(3)
    n = 2000
    u, v = rng.uniform(0.4, 0.6, n), rng.uniform(0.4, 0.6, n)
    dx, dy = rng.uniform(-0.3, 0.3, (2, n)), rng.uniform(-0.08, 0.08, (2, n))
    rgb, N, L, _ = X.sample(T.BASE.tex(), u, v, dx[0], dx[1], dy[0], dy[1], ft=np.float64)
    assert set(N.tolist()) >= {2, 3, 4} and L.max() > 256 and np.abs(rgb - T.BASE.value(u, v)[:, :3]).max() < 1e-12


# ---- the scenes ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", R.TARGETS)
@pytest.mark.parametrize("name", sorted(T.SCENES))
def test_left_out_share_is_under_the_cap(record_property, name, w, h):
    _, rc = T.cast_scene(name, w, h)
    for forward in ([False, True] if name in T.FORWARD_SCENES else [False]):
        compared, any_hit, share = T.classify(rc, forward)
        record_property(f"{name} {w}x{h}{' forward' if forward else ''}: left-out share", round(share, 4))
        print(f"{name} {w}x{h} forward={forward}: {int(any_hit.sum())} texels hit, {int((any_hit & compared).sum())} compared, left out {share:.4f}")
        assert any_hit.sum() >= w * h // 8 and share <= R.LEFT_OUT_CAP


def test_scenes_are_what_they_claim():
    for w, h in R.TARGETS:
        sc = T.textured_scene(w, h)
        keys = [m["key"] for m in sc.mats]
        assert 15 in keys and all(any(k & b for k in keys) and any(not k & b for k in keys) for b in (1, 2, 4, 8))
        assert sc.mats[1]["base_color"].srgb and sc.mats[0]["base_color"].kind == "ramp"
        assert {float(np.ascontiguousarray(d.vertices).view(F).reshape(-1, 16)[0, 11]) for d in sc.draws} == {-1.0, 1.0}
        for s in (sc, T.textured_strip_scene(w, h), T.masked_scene(w, h)):
            for d in s.draws:
                t = [d.transforms[n] for n in T.NAMES if n in d.transforms]
                assert len({tuple(np.round(np.concatenate([np.ravel(x) for x in tr]), 6)) for tr in t}) == len(t)  # every map its own transform
                uv = np.ascontiguousarray(d.vertices).view(F).reshape(-1, 16)[:, 6:8].astype(np.float64)
                assert uv.min() >= 0.3 - 1e-6 and uv.max() <= 0.7 + 1e-6
                for n in d.transforms:
                    c = T.transform(d, n, uv)
                    assert c.min() > 0.1 and c.max() < 0.9, (s.name, n, c.min(), c.max())
        # the levels scene: the compared texels span levels 0 to 3 and every N from 2 to 4
        _, rc = T.cast_scene("levels", w, h)
        at = T.classify(rc)[0] & rc["hit"][0]
        L = np.concatenate([rc["level_" + n][0][at] for n in ("emissive", "metallic_roughness")])
        N = np.concatenate([rc["N_" + n][0][at] for n in ("emissive", "metallic_roughness")])
        assert L.min() == 0.0 and L.max() == 3.0 and all(((L > k) & (L < k + 1)).sum() >= 10 for k in range(3)), np.histogram(L, bins=6)
        assert all((N == k).sum() >= 20 for k in (2, 3, 4)), np.bincount(N.astype(int))
        # the masked scene: winners behind one and behind two discarded hits, a masked winner, and the background through both
        sc, rc = T.cast_scene("masked", w, h)
        compared = T.classify(rc)[0]
        hit, gone = rc["hit"][0] & compared, rc["discards"][0]
        assert (hit & (gone == 1)).sum() >= 50 and (hit & (gone == 2)).sum() >= 50 and (compared & ~rc["hit"][0] & (gone == 2)).sum() >= 50
        for k in sc.masked:  # each masked draw wins somewhere and loses a band of itself
            assert (hit & (rc["draw"][0] == k)).sum() >= 50 and ((rc["signature"][0] >> np.arange(0, 12, 4)[:, None, None]) & 15 == k + 1).any()
        assert not sc.mats[2]["key"] & X.BASE_COLOR and sc.mats[1]["key"] & X.BASE_COLOR


# ---- the restatements against the ray caster ------------------------------------------------------------------------------------------------

def passes(sc, w, h, draws=None, mats=None, frame=None, plant=None):
    """(depth in front, the G-buffer restatement's dict - masked_pass' with a masked selection -, forward_pass' dict if a frame is given)."""
    draws = sc.draws if draws is None else draws
    mats = T.ref_materials(sc.mats if mats is None else mats)
    opaque, masked = [(k, k) for k in sc.opaque], [(k, k) for k in sc.masked]
    depth, _ = D.depth_prepass(draws, sc.view, sc.proj, w, h, slots=sc.opaque)
    if sc.masked:
        out = M.masked_pass(draws, sc.view, sc.proj, depth, w, h, materials=mats, select=opaque, mask_select=masked)
    else:
        out = X.gbuffer_pass(draws, sc.view, sc.proj, depth, w, h, materials=mats)
    fwd = None
    if frame is not None:
        fwd = FW.forward_pass(draws, sc.view, sc.proj, depth, w, h, frame, materials=mats, select=opaque, mask_select=masked if sc.masked else None,
                              hdr=T.background(w, h), plant=plant)
    return depth, out, fwd


_RESTATED = {}


def restated(name, w, h):
    if (name, w, h) not in _RESTATED:
        sc, _ = T.cast_scene(name, w, h)
        _RESTATED[(name, w, h)] = passes(sc, w, h, frame=T.scene_frame(sc) if name in T.FORWARD_SCENES else None)
    return _RESTATED[(name, w, h)]


def held(sc, rc, out):
    res = T.compare_masked(rc, out, sc.draws, sc.masked) if sc.masked else T.compare_gbuffer(rc, out, sc.draws)
    if sc.name == "levels":
        res.update(T.compare_levels(rc, out))
    return res


@pytest.mark.parametrize("w,h", R.TARGETS)
@pytest.mark.parametrize("name", sorted(T.SCENES))
def test_gbuffer_restatement_agrees(record_property, name, w, h):
    sc, rc = T.cast_scene(name, w, h)
    res = held(sc, rc, restated(name, w, h)[1])
    report(record_property, f"{'masked_pass' if sc.masked else 'gbuffer_pass'}, {name} {w}x{h}", res)
    assert R.failures(res) == 0, res


@pytest.mark.parametrize("w,h", R.TARGETS)
@pytest.mark.parametrize("name", T.FORWARD_SCENES)
def test_forward_restatement_agrees(record_property, name, w, h):
    _, rc = T.cast_scene(name, w, h)
    res = T.compare_forward(rc, restated(name, w, h)[2]["hdr"], T.background(w, h))
    report(record_property, f"forward_pass, {name} {w}x{h}", res)
    assert R.failures(res) == 0, res


# ---- detectors: a planted error must fail the output it touches and blame nothing else -------------------------------------------------------

def blamed(res):
    return {k for k, (fails, _) in res.items() if fails}


def _with_vertices(d, change):
    d = copy.copy(d)
    v = np.ascontiguousarray(d.vertices).view(F).reshape(-1, 16).copy()
    change(v)
    d.vertices = v.reshape(-1).view(np.uint8).copy()
    return d


def _with_transforms(d, change):
    d = copy.copy(d)
    d.transforms = change(dict(d.transforms))
    return d


def test_detector_metallic_from_g():
    """The metallic-roughness map with G and B exchanged is what a resolve that reads metallic from .g and roughness from .b sees."""
    sc, rc = T.cast_scene("textured", W0, H0)
    mats = T.ref_materials(sc.mats)
    for m in mats:
        m["metallic_roughness"] = X.Tex([lv[:, :, [0, 2, 1, 3]] for lv in m["metallic_roughness"].levels])
    res = held(sc, rc, passes(sc, W0, H0, mats=mats)[1])
    assert blamed(res) == {"B.yz"} and res["B.yz"][1] > 1.0, res


def test_detector_exchanged_transforms():
    sc, rc = T.cast_scene("textured", W0, H0)
    swap = lambda t: dict(t, metallic_roughness=t["emissive"], emissive=t["metallic_roughness"])  # noqa: E731
    res = held(sc, rc, passes(sc, W0, H0, draws=[_with_transforms(d, swap) for d in sc.draws])[1])
    assert blamed(res) == {"B.yz", "hdr"}, res


def test_detector_negated_sine():
    """The base-colour transform's rotation taken the other way round: C alone moves."""
    sc, rc = T.cast_scene("textured", W0, H0)
    flip = lambda t: dict(t, base_color=(t["base_color"][0], t["base_color"][1], (t["base_color"][2][0], -t["base_color"][2][1])))  # noqa: E731
    res = held(sc, rc, passes(sc, W0, H0, draws=[_with_transforms(d, flip) for d in sc.draws])[1])
    assert blamed(res) == {"C"} and res["C"][1] > 1.0, res


def test_detector_tangent_w_ignored():
    sc, rc = T.cast_scene("textured", W0, H0)

    def positive(v):
        v[:, 11] = 1.0

    res = held(sc, rc, passes(sc, W0, H0, draws=[_with_vertices(d, positive) for d in sc.draws])[1])
    assert blamed(res) == {"A"} and res["A"][1] > 1.0, res


def test_detector_forward_normal_with_reconstructed_z(monkeypatch):
    """The forward resolve handed a normal map whose third channel is the base pass' reconstructed z: hdr moves, the G-buffer does not."""
    sc, rc = T.cast_scene("textured", W0, H0)
    right = X.sample

    def wrong(tex, *a, **kw):
        rgb, N, L, taps = right(tex, *a, **kw)
        if tex.levels[0][0, 0, 2] == 250:  # (the normal ramp: its B starts at 250)
            r, g = rgb[:, 0] * 2 - 1, rgb[:, 1] * 2 - 1
            rgb = rgb.copy()
            rgb[:, 2] = (np.sqrt(np.clip(1 - (r * r + g * g), 0, 1)) + 1) / 2
        return rgb, N, L, taps

    assert T.NORMAL.tex().levels[0][0, 0, 2] == 250 and all(a.tex().levels[0][0, 0, 2] != 250 for a in (T.BASE, T.METAL_ROUGH, T.EMISSIVE))
    monkeypatch.setattr(X, "sample", wrong)
    _, out, fwd = passes(sc, W0, H0, frame=T.scene_frame(sc))
    assert blamed(held(sc, rc, out)) == set()  # (the base pass never reads the third channel)
    res = T.compare_forward(rc, fwd["hdr"], T.background(W0, H0))
    assert blamed(res) == {"hdr"} and res["hdr"][1] > 1.0, res


def test_detector_alpha_without_vertex_alpha():
    sc, rc = T.cast_scene("masked", W0, H0)

    def opaque_alpha(v):
        v[:, 15] = 1.0

    res = held(sc, rc, passes(sc, W0, H0, draws=[_with_vertices(d, opaque_alpha) for d in sc.draws])[1])
    assert {"depth", "A", "C", "won"} <= blamed(res), res  # the grid is never discarded: another draw wins, nearer


def test_detector_discarded_fragment_writes_depth():
    """The depth of a pass that discards nothing (every cutoff 0) in place of the right one: what a discarded fragment that still wrote
    depth leaves behind. The G-buffer outputs are the right pass' and stay."""
    sc, rc = T.cast_scene("masked", W0, H0)
    draws = []
    for d in sc.draws:
        d = copy.copy(d)
        d.cutoff = 0.0
        draws.append(d)
    out = dict(restated("masked", W0, H0)[1], depth=passes(sc, W0, H0, draws=draws)[1]["depth"])
    res = held(sc, rc, out)
    assert blamed(res) == {"depth", "depth covered"} and res["depth"][1] > 1.0, res


def _levels_with(monkeypatch, wrong_level):
    """The levels scene with gbuffer_tex_ref.sample's level of a level-coded map replaced: such a map's sample is 60 (L / 256) / 255
    whatever else the sampler does, so the planted sampler returns that for wrong_level(pmax2, N, mips)."""
    sc, rc = T.cast_scene("levels", W0, H0)
    right = X.sample

    def wrong(tex, u, v, dxu, dxv, dyu, dyv, ft=np.float32):
        rgb, N, L, taps = right(tex, u, v, dxu, dxv, dyu, dyv, ft)
        if len(tex.levels) == 4 and int(tex.levels[3][0, 0, 0]) == 180 and int(tex.levels[0][5, 7, 1]) == 0:  # a level-coded chain
            with np.errstate(all="ignore"):
                px2 = (dxu * ft(tex.width)) ** 2 + (dxv * ft(tex.height)) ** 2
                py2 = (dyu * ft(tex.width)) ** 2 + (dyv * ft(tex.height)) ** 2
                L = wrong_level(np.maximum(px2, py2).astype(ft), N, len(tex.levels))
            rgb = np.repeat((ft(60.0) * (L.astype(ft) / ft(256.0)) / ft(255.0))[:, None], 3, axis=1).astype(ft)
        return rgb, N, L, taps

    monkeypatch.setattr(X, "sample", wrong)
    return held(sc, rc, passes(sc, W0, H0)[1])


def test_detector_level_from_rho_squared(monkeypatch):
    """256 log2(rho^2) in place of 256 log2(rho): twice the level."""
    res = _levels_with(monkeypatch, lambda pmax2, N, mips: X.level_of_detail((pmax2 / (N * N).astype(pmax2.dtype)) ** 2, mips))
    assert blamed(res) == {"B.yz", "hdr", "level B", "level hdr"}, res


def test_detector_rho_without_the_division_by_n(monkeypatch):
    res = _levels_with(monkeypatch, lambda pmax2, N, mips: X.level_of_detail(pmax2, mips))
    assert blamed(res) == {"B.yz", "hdr", "level B", "level hdr"}, res


def test_detector_planted_sampler_alone_changes_nothing(monkeypatch):
    res = _levels_with(monkeypatch, lambda pmax2, N, mips: X.level_of_detail(pmax2 / (N * N).astype(pmax2.dtype), mips))
    assert blamed(res) == set(), res
