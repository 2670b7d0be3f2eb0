"""The numpy restatement of Build HZB and CullIndirectArgs (tests/visibility_ref.py) pinned by hand-derived answers, held
against the CPU oracle on random and edge inputs, and shown to separate planted errors that the random inputs miss."""
import math

import numpy as np
import pytest

from tests import visibility_ref as V
from unclerenderer_amd import hostmath, synth

F = np.float32


@pytest.fixture(scope="module")
def sets():
    return V.all_sets()


def _hz(s, layout):
    return V.hzb_flat(s["levels"], layout)[0] if s["levels"] is not None else None


# ---------------------------------------------------------------------------------------------------------------------
# arithmetic the restatement relies on
# ---------------------------------------------------------------------------------------------------------------------
def test_fp_environment(urlib):
    """numpy float32 stays correctly rounded with denormals kept, after torch and the project's libraries are loaded."""
    import torch  # noqa: F401  (loaded on purpose: it must not have changed the FP control state)
    tiny = np.array([1], np.uint32).view(F)[0]
    assert tiny > 0 and tiny * F(2) == np.array([2], np.uint32).view(F)[0]
    assert F(2.0 ** -126) / F(2) == np.array([0x00400000], np.uint32).view(F)[0]  # a denormal quotient, not flushed
    assert np.array([0x00800000], np.uint32).view(F)[0] - np.array([0x007FFFFF], np.uint32).view(F)[0] == tiny
    assert F(1) + F(2.0 ** -24) == F(1) and F(1) + F(2.0 ** -23) == np.nextafter(F(1), F(2))  # round to nearest even
    assert F(1) + F(3 * 2.0 ** -24) == F(1) + F(2.0 ** -22)
    a, c = F(1) + F(2.0 ** -12), F(1) + F(2.0 ** -11)
    assert a * a - c == F(0) and float(a) * float(a) - float(c) == 2.0 ** -24  # the product rounds (a tie, to even)
    assert F(1) / F(3) == np.float32(1.0 / 3.0)


def test_hmin_rule():
    nan = [V.SNAN, V.QNAN, V.NQNAN]
    for n in nan:
        assert V.hmin(n, F(0.5)) == F(0.5) and V.hmin(F(0.5), n) == F(0.5)
        assert V.hmax(n, F(0.5)) == F(0.5)
        assert np.isnan(V.hmin(n, n))
    assert np.isnan(V.glibc_fmin(V.SNAN, F(0.5))) and V.glibc_fmin(V.QNAN, F(0.5)) == F(0.5)
    v, free = V.min4(F(0.0), F(-0.0), F(1), F(1))
    assert v == 0 and free
    v, free = V.min4(F(-0.0), F(-0.0), F(1), V.SNAN)
    assert v == 0 and np.signbit(v) and not free
    assert np.isnan(V.min4(V.SNAN, V.QNAN, V.NQNAN, V.SNAN)[0])
    keys = V.ordered(np.array([-np.inf, -1, -0.0, 0.0, V.DENORM_MIN, 1, np.inf], F))
    assert (np.diff(keys) > 0).all() and keys[3] - keys[2] == 1 and keys[4] - keys[3] == 1
    x = np.array([-3.5, -0.0, 0.0, 1e-40, 7.0], F)
    assert np.array_equal(V.from_ordered(V.ordered(x)).view(np.uint32), x.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------
# Build HZB
# ---------------------------------------------------------------------------------------------------------------------
def test_hzb_known_answers():
    lv = V.build_hzb(np.array([[0.4, 0.9], [0.7, 0.2]], F))
    assert lv[0][0].tolist() == [[F(0.2)]]
    d = (np.arange(15, dtype=F).reshape(5, 3) + 1) / 16  # 3x5: clamped reads, then a floor halving that drops row 2
    m = [x for x, _ in V.build_hzb(d)]
    assert [x.shape for x in m] == [(3, 2), (1, 1)]
    assert m[0][2, 1] == d[4, 2] and m[1][0, 0] == d[:4].min()
    # H8: 17x9 -> 9x5, 4x2, 2x1, 1x1 in one dispatch; the 1x1 reads an out-of-range 0.0 slot
    m = [x for x, _ in V.build_hzb(np.full((9, 17), 0.5, F))]
    assert [x.shape for x in m] == [(5, 9), (2, 4), (1, 2), (1, 1)] and m[3][0, 0] == 0.0 and (m[2] == 0.5).all()
    # the HLSL min: an sNaN anywhere in a footprint is ignored; an all-NaN footprint stays NaN
    for s in range(4):
        d = np.full((2, 2), 0.75, F)
        d[s // 2, s % 2] = V.SNAN
        d[(s + 1) % 4 // 2, (s + 1) % 2] = F(0.25)
        assert V.build_hzb(d)[0][0][0, 0] == F(0.25)
    assert np.isnan(V.build_hzb(np.full((2, 2), V.SNAN, F))[0][0][0, 0])
    v, free = V.build_hzb(np.array([[0.0, -0.0], [0.5, 0.5]], F))[0]
    assert v[0, 0] == 0 and free[0, 0]
    v, free = V.build_hzb(np.array([[-0.0, -0.0], [0.5, 0.5]], F))[0]
    assert v[0, 0] == 0 and np.signbit(v[0, 0]) and not free[0, 0]


@pytest.mark.parametrize("w,h", [(1, 1), (3, 5), (17, 9), (64, 64), (129, 67), (640, 360), (1000, 3), (5, 300)])
def test_hzb_matches_oracle(oracle, w, h):
    layout = V.packed_layout(w, h)
    mips, total = oracle.hzb_layout(w, h)
    assert [tuple(m) for m in mips] == layout
    for depth in (np.random.default_rng(w * 31 + h).random((h, w), dtype=F), V.special_depth(w, h, seed=w + h)):
        want, free = V.hzb_flat(V.build_hzb(depth), layout)
        got = oracle.build_hzb(depth, mips, total)
        ok = V.same_bits(got, want, free)
        assert ok.all(), f"{(~ok).sum()} texels differ, first at {np.flatnonzero(~ok)[:8]}"
    assert not V.build_hzb(np.random.default_rng(0).random((h, w), dtype=F))[0][1].any()


def test_hzb_fmin_mutant_is_caught_by_special_depth_only():
    depth = np.random.default_rng(5).random((67, 129), dtype=F)
    lay = V.packed_layout(129, 67)
    a, _ = V.hzb_flat(V.build_hzb(depth), lay)
    b, _ = V.hzb_flat(V.build_hzb(depth, fmin=V.glibc_fmin), lay)
    assert V.same_bits(a, b).all()
    d = V.special_depth(129, 67)
    a, fa = V.hzb_flat(V.build_hzb(d), lay)
    b, _ = V.hzb_flat(V.build_hzb(d, fmin=V.glibc_fmin), lay)
    assert not V.same_bits(b, a, fa).all()


# ---------------------------------------------------------------------------------------------------------------------
# Cull: known answers (the boxes of test_oracle_kat.py, restated)
# ---------------------------------------------------------------------------------------------------------------------
def _simple():
    view = np.eye(4, dtype=F).ravel()
    proj = hostmath.reverse_z_projection(math.radians(90.0), 1.0, 0.1)
    return view, proj


def _box(cx, cy, cz, e=0.5):
    return V.boxes(np.array([[cx, cy, cz]], F), np.full((1, 3), e, F))[0]


def _hzb_const(values, w=8, h=8):
    lay = V.packed_layout(w, h)
    sizes = V.hzb_sizes(w, h)
    return lay, V.hzb_flat([(np.full((mh, mw), v, F), None) for (mw, mh), v in zip(sizes, values)], lay)[0]


def test_cull_frustum_known_answers():
    view, proj = _simple()
    boxes = {"centre": (_box(0, 0, 5), 1), "right": (_box(10, 0, 5), 0), "left": (_box(-10, 0, 5), 0), "above": (_box(0, 10, 5), 0),
             "below": (_box(0, -10, 5), 0), "behind": (_box(0, 0, -5), 0), "straddles right": (_box(5, 0, 5), 1),
             "straddles near": (_box(0, 0, 0.1), 1), "just outside right": (_box(6.01, 0, 5.0), 0), "touching right": (_box(6.0, 0, 5.0), 1),
             "far away": (_box(0, 0, 1e6, 10.0), 1), "contains camera": (_box(0, 0, 0, 3.0), 1)}
    b = np.stack([x for x, _ in boxes.values()])
    c = hostmath.pack_culling_constants(view, proj, len(boxes), False, 0, 0, 0, True)
    r = V.cull(c, b)
    assert r["visible"].astype(int).tolist() == [v for _, v in boxes.values()]


def test_cull_occlusion_known_answers():
    view, proj = _simple()
    one = _box(0, 0, 5)[None]
    max_depth = F(F(0.1) / F(4.5))

    def run(bounds, values):
        lay, hz = _hzb_const(values)
        c = hostmath.pack_culling_constants(view, proj, bounds.shape[0], True, len(lay), lay[0][1], lay[0][2], True)
        return V.cull(c, bounds, hz, lay)

    assert not run(one, [0.5] * 3)["visible"][0]
    assert run(one, [0.01] * 3)["visible"][0]
    r = run(one, [max_depth] * 3)
    assert r["maxDepth"][0] == max_depth and r["visible"][0]  # equality: maxDepth < hzbDepth is false
    assert not run(one, [np.nextafter(max_depth, F(1))] * 3)["visible"][0]
    span = np.zeros((1, 2, 4), F)
    span[0, 0, :3], span[0, 1, :3] = [-0.5, -0.5, -1.0], [0.5, 0.5, 5.0]
    r = run(span, [1.0] * 3)
    assert r["behind"][0] and r["visible"][0]
    assert run(one, [0.0, 0.5, 1.0])["mip"][0] == 0
    r = run(_box(0, 0, 5, 4.6)[None], [0.0, 0.5, 1.0])
    assert r["mip"][0] == 2 and not r["visible"][0]
    assert run(_box(0, 0, 5, 1.5)[None], [0.0, 1.0, 1.0])["mip"][0] == 0
    assert run(_box(0, 0, 5, 2.0)[None], [0.0, 1.0, 0.0])["mip"][0] == 1
    # the HLSL min over the taps: a signalling or quiet NaN texel is ignored, an all-NaN rect leaves hzbDepth at 1.0
    for bad in (V.SNAN, V.QNAN, V.NQNAN):
        r = run(one, [bad, 0.5, 0.5])
        assert r["hzbDepth"][0] == 1.0 and not r["visible"][0]
        assert r["maxDepth"][0] < 1.0
        lay, hz = _hzb_const([bad] * 3)
        c = hostmath.pack_culling_constants(view, proj, 1, True, len(lay), lay[0][1], lay[0][2], True)
        assert V.cull(c, one, hz, lay)["hzbDepth"][0] == 1.0  # every tap NaN: hzbDepth stays 1.0
        assert V.cull(c, one, hz, lay, mutant="fmin")["visible"][0] == (bad is V.SNAN)  # glibc's rule: an sNaN tap gives NaN
    r = run(one, [-0.0, 0.5, 0.5])
    assert r["hzbDepth"][0] == 0 and r["visible"][0]


def test_offscreen_early_out_is_unreachable(sets):
    """minUv starts at (1, 1) and maxUv at (0, 0), and HLSL min / max ignore NaN: `maxUv < 0 || minUv > 1` never holds.
    A box wholly off screen is tested against the edge texels instead."""
    rng = np.random.default_rng(3)
    b = np.zeros((20000, 2, 4), F)
    b[:, 0, :3] = rng.normal(0, 1e3, (20000, 3)).astype(F)
    b[:, 1, :3] = b[:, 0, :3] + rng.uniform(0, 10, (20000, 3)).astype(F)
    cam = V.dyadic_camera()
    lay = V.packed_layout(*V.HZB_SRC)
    hz, _ = V.hzb_flat(V.mip_fill(F(1.0)), lay)
    r = V.cull(V.constants(V.PERMISSIVE, cam["vp"], 20000, True, len(lay), lay[0][1], lay[0][2]), b, hz, lay)
    assert not r["offscreen"].any() and (~r["behind"]).sum() > 1000
    sp = [s for s in sets if s["name"] == "specials/permissive"][0]
    r = V.cull(V.with_count(sp["consts"], sp["bounds"].shape[0]), sp["bounds"], _hz(sp, lay), lay)
    assert not r["visible"][-4:].any() and r["tested"][-4:].all()  # the four off-screen boxes: occluded by the 0.5 edge texels


# ---------------------------------------------------------------------------------------------------------------------
# Cull: the restatement against the oracle
# ---------------------------------------------------------------------------------------------------------------------
def _random_cases(oracle):
    """The random sets of the GPU parity tests: the Sponza camera, a scene HZB, instances_random."""
    out = []
    for n, seed, hzb_on in ((4097, 4104, True), (100_000, 100_007, True), (20_000, 20_007, False), (5000, 99, True)):
        w, h = 480, 270
        fc = hostmath.build_frame_constants("sponza", w, h)
        g = synth.gbuffer_scene(fc.view, fc.proj, fc.camera_position, w, h, seed)
        lay = V.packed_layout(w, h)
        mips, total = oracle.hzb_layout(w, h)
        hz = np.nan_to_num(oracle.build_hzb(g.depth, mips, total), nan=0.0)
        b = synth.instances_random(n, seed, center=fc.camera_position, box=120.0)
        c = hostmath.pack_culling_constants(fc.view, fc.proj, n, hzb_on, len(lay), lay[0][1], lay[0][2], True)
        out.append((c, b, hz, lay))
    return out


def test_cull_matches_oracle_on_random_sets(oracle):
    for c, b, hz, lay in _random_cases(oracle):
        n = int(c[40])
        want = V.expected_outputs(c, b, hz, lay, synth.indirect_args_initial(n))
        got = oracle.cull_indirect_args(c, b, hz, lay, synth.indirect_args_initial(n))
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]) and got[3] == want[3]


def test_cull_matches_oracle_on_edge_sets(oracle, sets):
    lay = V.packed_layout(*V.HZB_SRC)
    for s in sets:
        b = s["bounds"]
        n = b.shape[0]
        c = V.with_count(s["consts"], n)
        hz = _hz(s, lay)
        want = V.expected_outputs(c, b, hz, lay, synth.indirect_args_initial(n))
        got = oracle.cull_indirect_args(c, b, hz if hz is not None else None, lay if hz is not None else [], synth.indirect_args_initial(n))
        bad = np.flatnonzero(got[0][:, 11] != want[0][:, 11])
        assert bad.size == 0, (s["name"], bad[:8])
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), s["name"]


def test_float32_restatement_agrees_with_float64_outside_the_band(oracle):
    total = inband = 0
    for c, b, hz, lay in _random_cases(oracle):
        r32 = V.cull(c, b, hz, lay)
        r64 = V.cull_f64(c, b, hz, lay)
        out = ~r64["band"]
        assert np.array_equal(r32["visible"][out], r64["visible"][out])
        total += b.shape[0]
        inband += int(r64["band"].sum())
    assert inband <= 0.001 * total, f"{inband} of {total} instances within the float32 error band"


# ---------------------------------------------------------------------------------------------------------------------
# the generator and the planted mutants
# ---------------------------------------------------------------------------------------------------------------------
# pairs each camera's sets must split, per decision kind (the Sponza and pica_pica far planes are NaN: a plane that passes
# everything, so no pair can split it)
MIN_PAIRS = {"plane0": 30, "plane1": 30, "plane2": 30, "plane3": 30, "plane5": 30, "depth": 30, "mip": 80, "clamp": 20, "minX": 5, "minY": 5,
             "maxX": 5, "maxY": 5, "saturate": 30}


def split_counts(sets):
    lay = V.packed_layout(*V.HZB_SRC)
    per = {}
    for s in sets:
        if s["kind"] in ("specials", "depth_eq"):
            continue
        key = s["cam"]["name"] if s["kind"] != "clip_w" else "clip_w"
        acc = per.setdefault(key, {})
        for k, v in V.classify(s["consts"], s["bounds"], _hz(s, lay), lay).items():
            acc[k] = acc.get(k, 0) + v
    return per


def test_generator_splits_every_decision_kind(sets):
    per = split_counts(sets)
    for cam in ("dyadic", "sponza", "pica_pica"):
        need = dict(MIN_PAIRS, **({"plane4": 30} if cam == "dyadic" else {}))
        short = {k: (per[cam].get(k, 0), m) for k, m in need.items() if per[cam].get(k, 0) < m}
        assert not short, (cam, short)
    assert per["clip_w"]["clip_w"] >= 100
    lay = V.packed_layout(*V.HZB_SRC)
    for s in sets:  # every pair really is two adjacent float32 inputs deciding differently
        if s["kind"] in ("specials", "depth_eq"):
            continue
        b = s["bounds"]
        r = V.cull(V.with_count(s["consts"], b.shape[0]), b, _hz(s, lay), lay)
        assert (r["visible"][0::2] != r["visible"][1::2]).all(), s["name"]


# A truncating texel conversion replaced by round-to-nearest moves taps by a whole texel for about a third of the tested
# instances: the random sets notice that one already. Every other mutant decides every random instance as the restatement.
NOTICED_BY_RANDOM_SETS = {"round"}


@pytest.mark.parametrize("mutant", V.MUTANTS)
def test_mutant_caught_on_edge_sets_missed_on_random_sets(oracle, sets, mutant):
    differ = sum(int((V.cull(c, b, hz, lay, mutant)["visible"] != V.cull(c, b, hz, lay)["visible"]).sum()) for c, b, hz, lay in _random_cases(oracle))
    assert (differ > 0) == (mutant in NOTICED_BY_RANDOM_SETS), differ
    lay = V.packed_layout(*V.HZB_SRC)
    caught = 0
    for s in sets:
        n = s["bounds"].shape[0]
        c = V.with_count(s["consts"], n)
        hz = _hz(s, lay)
        caught += int((V.cull(c, s["bounds"], hz, lay, mutant)["visible"] != V.cull(c, s["bounds"], hz, lay)["visible"]).sum())
    assert caught > 0, f"mutant {mutant} decides every edge instance as the restatement does"
