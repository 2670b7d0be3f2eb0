"""Footprints of Build HZB and CullIndirectArgs (csrc/hzb.hip, hzb_wide.h, hzb_tail.h, cull.hip, cull_views.hip) under the rules of
tests/footprint.py: the depth buffer of odd-sized frames read in wide rows, the band form writing only its five slices, the riding
chain writing from inside a Lighting launch, and the cull's words, list, stats, masks and command slots with everything the header
leaves alone still holding its fill. Nothing here judges a value."""
import numpy as np
import pytest

from tests import footprint as F

pytestmark = pytest.mark.gpu

HZB_SIZES = [(1, 1), (17, 9), (129, 67), (1918, 1082), (3840, 2160), (6001, 3999)]


def _depth(w, h, seed):
    rng = np.random.default_rng(seed)
    d = rng.random((h, w), dtype=np.float32)
    d[rng.random((h, w)) < 0.1] = 0.0
    return d


def _hzb_fill(total, seed):
    return np.random.default_rng(seed).random(total, dtype=np.float32) + 2.0


def _gaps(lay):
    """Floats of the HZB allocation that belong to no mip (the mips sit on 256-byte boundaries)."""
    m = np.ones(lay.total, bool)
    for (o, w, h) in lay.as_list():
        m[o:o + w * h] = False
    return m


@pytest.mark.parametrize("w,h", HZB_SIZES)
def test_build_hzb_footprint(hotpath, w, h):
    """ur_build_hzb: depth of exactly w * h floats, the HZB of exactly ur_hzb_layout's total; the floats between the mips are not written."""
    from unclerenderer_amd.hotpath import HzbLayout
    lay = HzbLayout(w, h)
    gaps = _gaps(lay)
    F.run_rules(lambda b: hotpath.build_hzb(b["depth"], b["hzb"], lay), {"depth": _depth(w, h, w)}, {"hzb": _hzb_fill(lay.total, h)},
                row_bytes={"hzb": lay.width * 4}, untouched=lambda r: {"hzb": gaps}, what=f"build_hzb {w}x{h}")


@pytest.mark.parametrize("w,h,world", [(1918, 1080, 2), (1918, 1080, 3), (1918, 1080, 8), (3840, 2160, 8)])
def test_build_hzb_band_and_tail_footprint(hotpath, w, h, world):
    """ur_build_hzb_band for every rank (ur_hzb_band_pieces wants the ranks to divide the rows): only the band's five slices of mips 0..4 are written. ur_build_hzb_tail: mips 0..4 are read
    and stay as they are, only mips 5.. are written."""
    from unclerenderer_amd.hotpath import HzbLayout
    lay = HzbLayout(w, h)
    depth, fill = _depth(w, h, world), _hzb_fill(lay.total, 3)
    whole = fill.copy()
    for r in range(world):
        p0, pn = lay.band_pieces(world, r)
        outside = np.ones(lay.total, bool)
        for off, cnt in lay.band_slices(p0, pn):
            outside[off:off + cnt] = False
        got = F.run_rules(lambda b: hotpath.build_hzb_band(b["depth"], b["hzb"], lay, p0, pn), {"depth": depth}, {"hzb": fill},
                          row_bytes={"hzb": lay.width * 4}, untouched=lambda r_: {"hzb": outside}, what=f"build_hzb_band {w}x{h} rank {r}/{world}")
        whole[~outside] = got["hzb"][~outside]
    head = np.zeros(lay.total, bool)
    o5 = lay.as_list()[5][0]
    head[:o5] = True
    F.run_rules(lambda b: hotpath.build_hzb_tail(b["hzb"], lay), {}, {"hzb": whole}, row_bytes={"hzb": lay.width * 4},
                untouched=lambda r_: {"hzb": head | _gaps(lay)}, what=f"build_hzb_tail {w}x{h}")


@pytest.mark.parametrize("mode", [1, 2])
def test_build_hzb_riding_lighting_footprint(hotpath, mode):
    """ur_defer_hzb_tail 1 and 2 behind a streaming Lighting launch (ur_build_hzb, and the pieces of ur_build_hzb_band riding under
    mode 2): depth, HZB, the G-buffer and the HDR target all guarded."""
    from tests.test_gpu_parity import _device_tables, _lighting_inputs
    from unclerenderer_amd.hotpath import HzbLayout
    w, h = 1024, 512
    fc, g, shadow, env, lut = _lighting_inputs("sponza", w, h, seed=5, mode="scene")
    tables = _device_tables(hotpath, shadow, env, lut)
    lay = HzbLayout(w, h)
    gaps = _gaps(lay)
    ins = {"A": g.A, "B": g.B, "C": g.C, "D": g.depth, "hzb_depth": _depth(w, h, 6)}
    pieces = [None, lay.band_pieces(2, 1)] if mode == 2 else [None]
    for band in pieces:
        def call(b):
            hotpath.defer_hzb_tail(mode)
            try:
                if band is None:
                    hotpath.build_hzb(b["hzb_depth"], b["hzb"], lay)
                else:
                    hotpath.build_hzb_band(b["hzb_depth"], b["hzb"], lay, *band)
                hotpath.deferred_lighting_sky(fc.scene, fc.sky, b["A"], b["B"], b["C"], b["D"], tables, b["hdr"], w, h)
                if band is None:
                    assert mode == 1 or hotpath.lighting_schedule()["hzb_pieces"] > 0
            finally:
                hotpath.defer_hzb_tail(0)
        outside = gaps.copy()
        if band is not None:
            outside[:] = True
            for off, cnt in lay.band_slices(*band):
                outside[off:off + cnt] = False
        F.run_rules(call, ins, {"hzb": _hzb_fill(lay.total, 7), "hdr": g.hdr}, row_bytes={"hzb": lay.width * 4},
                    untouched=lambda r: {"hzb": outside}, what=f"riding mode {mode} band {band}")
    hotpath.flush()


def _cull_setup(hotpath, n, seed=3):
    """Bounds around sponza's camera, culling constants and an HZB the GPU built (640 x 360), read back."""
    import torch
    from unclerenderer_amd import hostmath, synth
    from unclerenderer_amd.hotpath import HzbLayout, to_device
    w, h = 640, 360
    fc = hostmath.build_frame_constants("sponza", w, h)
    g = synth.gbuffer_scene(fc.view, fc.proj, fc.camera_position, w, h, seed)
    lay = HzbLayout(w, h)
    hzb = torch.zeros(lay.total, device="cuda")
    hotpath.build_hzb(to_device(g.depth), hzb, lay)
    torch.cuda.synchronize()
    bounds = synth.instances_random(max(n, 1), seed, center=fc.camera_position, box=60.0)
    return fc, lay, hzb.cpu().numpy(), bounds


def _args0(n, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 2 ** 32, size=(n, 16), dtype=np.uint32)
    a[:, 11] = rng.choice(np.array([0, 1, 7], np.uint32), size=n)
    return a


def _not_word_11(n):
    m = np.ones((n, 16), bool)
    m[:, 11] = False
    return m


CULL_COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 4097, 70_000]


@pytest.mark.parametrize("n", CULL_COUNTS)
def test_cull_footprint(hotpath, n):
    """ur_cull_indirect_args and ur_cull_indirect_args_ex (index_base): bounds of exactly 2 n float4, commands of exactly n * 64 bytes
    of which only the InstanceCount words change, the list of exactly n words untouched beyond *visible_count, stats2 of two words;
    with and without the list, with the HZB on and off. n = 0 passes one spare element per buffer, which stays as it is."""
    from unclerenderer_amd import hostmath
    fc, lay, hzb, bounds = _cull_setup(hotpath, n)
    m = max(n, 1)
    rng = np.random.default_rng(n)
    for hzb_on in (True, False):
        consts = hostmath.pack_culling_constants(fc.view, fc.proj, n, hzb_on, lay.count, lay.width, lay.height, True)
        for with_list in (True, False):
            for index_base in (0, 1_000_003):
                if index_base and not (with_list and hzb_on):
                    continue
                ins = {"bounds": bounds[:m], "hzb": hzb if hzb_on else None}
                outs = {"args": _args0(m, n), "stats": np.array([5, 9], np.uint32),
                        "vis": rng.integers(0, 2 ** 32, m, dtype=np.uint32) if with_list else None,
                        "cnt": np.array([0xFFFFFFFF], np.uint32) if with_list else None}

                def left_alone(r):
                    keep = {"args": _not_word_11(m)}
                    if n == 0:
                        keep["args"] = np.ones((m, 16), bool)
                    if with_list:
                        cnt = int(r["cnt"][0])
                        assert cnt <= n
                        keep["vis"] = np.arange(m) >= cnt
                    return keep

                got = F.run_rules(lambda b: hotpath.cull_indirect_args(consts, b["bounds"], b["hzb"], lay if hzb_on else None, b["args"], b["stats"],
                                                                       b["vis"], b["cnt"], index_base),
                                  ins, outs, aligns={"args": 16, "stats": 4, "cnt": 4, "vis": 4, "bounds": 16}, row_bytes={"hzb": lay.width * 4},
                                  untouched=left_alone, what=f"cull n {n} hzb {hzb_on} list {with_list} base {index_base}")
                if n >= 255 and with_list:
                    assert 0 < int(got["cnt"][0]) < n, "both outcomes must occur"
                # stats2 may be NULL
                if with_list and hzb_on and not index_base:
                    F.run_rules(lambda b: hotpath.cull_indirect_args(consts, b["bounds"], b["hzb"], lay, b["args"], None, b["vis"], b["cnt"]),
                                ins, {k: v for k, v in outs.items() if k != "stats"}, untouched=left_alone, what=f"cull n {n} no stats")


@pytest.mark.parametrize("flavour", [0, 1, 2, 3, 4])
def test_cull_store_flavours_footprint(hotpath, flavour):
    """ur_cull_indirect_args under every UR_OPT_CULL_STORE: two launches on the same buffer (the second of flavour 4 runs from the
    context's record), at a count inside one block and at counts that end inside a wave and a block."""
    from unclerenderer_amd import hostmath, lib
    for n in (200, 257, 4097):
        fc, lay, hzb, bounds = _cull_setup(hotpath, n, seed=flavour + 1)
        fc2 = hostmath.build_frame_constants("pica_pica", 640, 360)
        c1 = hostmath.pack_culling_constants(fc.view, fc.proj, n, True, lay.count, lay.width, lay.height, True)
        c2 = hostmath.pack_culling_constants(fc2.view, fc2.proj, n, False, lay.count, lay.width, lay.height, True)

        def call(b):
            hotpath.set_option(lib.UR_OPT_CULL_STORE, flavour)  # (setting it forgets the record: every run starts alike)
            hotpath.cull_indirect_args(c1, b["bounds"], b["hzb"], lay, b["args"], b["stats"])
            hotpath.cull_indirect_args(c2, b["bounds"], b["hzb"], lay, b["args"], b["stats"])
        try:
            F.run_rules(call, {"bounds": bounds, "hzb": hzb}, {"args": _args0(n, flavour), "stats": np.zeros(2, np.uint32)},
                        aligns={"stats": 4}, untouched=lambda r: {"args": _not_word_11(n)}, what=f"cull store {flavour} n {n}")
        finally:
            hotpath.set_option(lib.UR_OPT_CULL_STORE, 3)


@pytest.mark.parametrize("n", [1, 200, 257, 4097])
def test_cull_draws_and_views_read_rule(hotpath, n):
    """ur_cull_indirect_args_draws and ur_cull_indirect_args_views: the read rule for bounds, hzb and offsets (the outputs' guards are
    tests/test_gpu_cull_draws.py's and test_gpu_cull_views.py's subject; they are guarded here all the same). Commands 16-byte aligned;
    slots [offsets[r] + counts[r], offsets[r + 1]) keep their fill, mask words beyond ceil(n / 32) are untouched, bits beyond n are 0."""
    from unclerenderer_amd import hostmath
    fc, lay, hzb, bounds = _cull_setup(hotpath, n, seed=9)
    consts = hostmath.pack_culling_constants(fc.view, fc.proj, n, True, lay.count, lay.width, lay.height, True)
    planes = hostmath.frustum_planes(hostmath.light_view_projection(fc.scene_center, fc.scene_radius * 0.25, fc.light_direction))
    offsets = np.unique(np.array([0, n // 3, n // 2, n], np.uint32))
    if offsets.size < 2:
        offsets = np.array([0, n], np.uint32)
    R = offsets.size - 1
    words = (n + 31) // 32
    rng = np.random.default_rng(n)
    cmd_fill = lambda s: np.random.default_rng(s).integers(0, 2 ** 32, (n, 16), dtype=np.uint32)  # noqa: E731
    ins = {"bounds": bounds, "hzb": hzb, "offsets": offsets}
    outs = {"args": _args0(n, n), "stats": np.zeros(2, np.uint32), "vis": rng.integers(0, 2 ** 32, n, dtype=np.uint32),
            "cnt": np.array([77], np.uint32), "cmds": cmd_fill(1), "counts": np.full(R, 0xABCD, np.uint32),
            "vmask": rng.integers(0, 2 ** 32, words + 3, dtype=np.uint32), "vcmds": cmd_fill(2), "vcounts": np.full(R, 0xABCD, np.uint32)}

    def slots_left(cmds_name, counts):
        m = np.zeros((n, 16), bool)
        for r in range(R):
            m[int(offsets[r]) + int(counts[r]):int(offsets[r + 1])] = True
        return m

    def left_alone_draws(r):
        return {"args": _not_word_11(n), "vis": np.arange(n) >= int(r["cnt"][0]), "cmds": slots_left("cmds", r["counts"])}

    def left_alone(r):
        assert n % 32 == 0 or int(r["vmask"][words - 1]) >> (n % 32) == 0, "mask bits beyond ModelCount must be 0"
        return dict(left_alone_draws(r), vcmds=slots_left("vcmds", r["vcounts"]), vmask=np.arange(words + 3) >= words)

    al = {"args": 16, "cmds": 16, "vcmds": 16, "offsets": 4, "counts": 4, "vcounts": 4, "vmask": 4, "stats": 4, "cnt": 4, "vis": 4}

    def draws(b):
        hotpath.cull_indirect_args(consts, b["bounds"], b["hzb"], lay, b["args"], b["stats"], b["vis"], b["cnt"], 0,
                                   draw_offsets=b["offsets"], draw_commands=b["cmds"], draw_counts=b["counts"])

    def views(b):
        hotpath.cull_indirect_args(consts, b["bounds"], b["hzb"], lay, b["args"], b["stats"], b["vis"], b["cnt"], 0,
                                   draw_offsets=b["offsets"], draw_commands=b["cmds"], draw_counts=b["counts"],
                                   views=[dict(planes=planes, mask=b["vmask"][:words], draw_offsets=b["offsets"], draw_commands=b["vcmds"],
                                               draw_counts=b["vcounts"])])

    F.run_rules(draws, ins, {k: v for k, v in outs.items() if not k.startswith("v") or k == "vis"}, aligns=al, untouched=left_alone_draws,
                what=f"cull draws n {n}")
    F.run_rules(views, ins, outs, aligns=al, untouched=left_alone, what=f"cull views n {n}")
