"""CullIndirectArgs and Build HZB on the GPU against the shader restatement (tests/visibility_ref.py) where kernels go wrong:
adjacent float32 inputs on either side of every cull decision, special texel and coordinate values, special-value depth
buffers in every launch form of the HZB chain, and the cull against HZBs the GPU built from those buffers.

Compared: the InstanceCount words and every other byte of the commands, the visible list, its count and the stats; per
draw range the commands and counts, with sentinels wherever nothing may be written. HZB texels bit for bit, NaN by NaN-ness
and zeros by value where the HLSL leaves the sign free."""
import numpy as np
import pytest

from tests import visibility_ref as V

pytestmark = pytest.mark.gpu

SENT = np.uint32(0xDEADBEEF)


def _torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def sets():
    return V.all_sets()


def _hzb_for(levels):
    """The edge HZB at the product's layout (mips on 256-byte boundaries), gaps filled with a sentinel."""
    from unclerenderer_amd.hotpath import HzbLayout
    lay = HzbLayout(*V.HZB_SRC)
    if levels is None:
        return lay, None, None
    buf, _ = V.hzb_flat(levels, lay.as_list())
    full = np.full(lay.total, SENT.view(np.float32), np.float32)
    for (o, w, h) in lay.as_list():
        full[o:o + w * h] = buf[o:o + w * h]
    return lay, full, lay.as_list()


def _args0(n, seed=0):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 2 ** 32, size=(n, 16), dtype=np.uint32)
    a[:, 11] = rng.choice(np.array([0, 1, 7], np.uint32), size=n)
    return a


def _cull(hotpath, consts, bounds, lay, hzb, args0, index_base=0, with_list=True):
    from unclerenderer_amd.hotpath import to_device
    torch = _torch()
    n = bounds.shape[0]
    d_args = to_device(args0)
    d_stats = torch.zeros(2, dtype=torch.int32, device="cuda")
    d_vis = torch.full((n + 64,), -1, dtype=torch.int32, device="cuda") if with_list else None
    d_cnt = torch.full((1,), -1, dtype=torch.int32, device="cuda") if with_list else None
    hotpath.cull_indirect_args(consts, to_device(bounds), to_device(hzb) if hzb is not None else None, lay if hzb is not None else None,
                               d_args, d_stats, d_vis, d_cnt, index_base)
    torch.cuda.synchronize()
    u = lambda t: t.cpu().numpy().view(np.uint32)  # noqa: E731
    return u(d_args).reshape(n, 16), u(d_stats), (u(d_vis) if with_list else None), (int(u(d_cnt)[0]) if with_list else None)


def _check(hotpath, oracle, consts, bounds, lay, hzb, layout, what, index_base=0, with_list=True, seed=0):
    n = bounds.shape[0]
    c = V.with_count(consts, n)
    args0 = _args0(n, seed)
    args, stats, vis, cnt = _cull(hotpath, c, bounds, lay, hzb, args0, index_base, with_list)
    want = V.expected_outputs(c, bounds, hzb, layout, args0, index_base)
    bad = np.flatnonzero(args[:, 11] != want[0][:, 11])
    assert bad.size == 0, f"{what}: {bad.size} InstanceCount words differ, first {bad[:8]}"
    assert np.array_equal(args, want[0]), f"{what}: bytes outside dword 11 changed"
    assert np.array_equal(stats, want[1]), what
    if with_list:
        assert cnt == want[3] and np.array_equal(vis[:cnt], want[2]), what
        assert (vis[cnt:] == 0xFFFFFFFF).all(), f"{what}: written past the list"
    # the CPU oracle decides the same (its NaN rule is the HLSL one)
    o = oracle.cull_indirect_args(c, bounds, hzb, layout if hzb is not None else [], args0, index_base)
    assert np.array_equal(o[0], want[0]), f"{what}: the oracle differs"
    return want


def test_cull_edges_single_block(hotpath, oracle, sets):
    """n <= 256: the single-block kernel, lane by lane."""
    for s in sets:
        lay, hzb, layout = _hzb_for(s["levels"])
        b = s["bounds"]
        for k in range(0, b.shape[0], 256):
            _check(hotpath, oracle, s["consts"], b[k:k + 256], lay, hzb, layout, f"{s['name']}[{k}:]")


def test_cull_edges_across_blocks_and_waves(hotpath, oracle, sets):
    """n >= 257: each set shuffled and tiled to an odd count, so that the packed occlusion test sees partial waves and pairs
    straddle wave and block boundaries; with index_base != 0, without the list, and with the HZB disabled."""
    rng = np.random.default_rng(11)
    for i, s in enumerate(sets):
        lay, hzb, layout = _hzb_for(s["levels"])
        b = s["bounds"]
        n = max(257, b.shape[0]) + 37 + i
        tiled = b[rng.permutation(np.resize(np.arange(b.shape[0]), n))]
        want = _check(hotpath, oracle, s["consts"], tiled, lay, hzb, layout, s["name"], seed=i)
        assert 0 < want[3] < n or s["kind"] == "specials", f"{s['name']}: both outcomes must occur"
        if i % 4 == 0:
            _check(hotpath, oracle, s["consts"], tiled, lay, hzb, layout, s["name"] + " base", index_base=1_000_003, seed=i)
            _check(hotpath, oracle, s["consts"], tiled, lay, hzb, layout, s["name"] + " no list", index_base=77, with_list=False, seed=i)
            off = V.with_count(s["consts"], n)
            off[41] = 0
            _check(hotpath, oracle, off, tiled, lay, hzb, layout, s["name"] + " hzb off", seed=i)


def test_cull_edges_beyond_4096_blocks(hotpath, oracle, sets):
    rng = np.random.default_rng(5)
    s = [x for x in sets if x["name"] == "mip/sponza"][0]
    lay, hzb, layout = _hzb_for(s["levels"])
    n = 4096 * 256 + 300
    b = s["bounds"][rng.integers(0, s["bounds"].shape[0], n)]
    c = V.with_count(s["consts"], n)
    args0 = np.zeros((n, 16), np.uint32)
    args0[:, 11] = 7
    args, stats, vis, cnt = _cull(hotpath, c, b, lay, hzb, args0)
    want = V.expected_outputs(c, b, hzb, layout, args0)
    assert np.array_equal(args, want[0]) and np.array_equal(stats, want[1])
    assert cnt == want[3] and np.array_equal(vis[:cnt], want[2])


@pytest.mark.parametrize("flavour", [0, 1, 2, 3, 4])
def test_cull_edges_store_flavours(hotpath, sets, flavour):
    """UR_OPT_CULL_STORE 0..4; 4 takes the old words from the record of a launch on the same buffer with another camera."""
    from unclerenderer_amd import lib
    from unclerenderer_amd.hotpath import to_device
    torch = _torch()
    s = [x for x in sets if x["name"] == "texel/pica_pica"][0]
    t = [x for x in sets if x["name"] == "texel/sponza"][0]
    lay, hzb, layout = _hzb_for(s["levels"])
    n = 2 * 256 + 45
    rng = np.random.default_rng(flavour)
    b = s["bounds"][rng.integers(0, s["bounds"].shape[0], n)]
    args0 = _args0(n, flavour)
    hotpath.set_option(lib.UR_OPT_CULL_STORE, flavour)
    try:
        d_args, d_b, d_h = to_device(args0), to_device(b), to_device(hzb)
        for consts in (t["consts"], s["consts"], t["consts"]):  # the first launch of the pair leaves the record the next one reads
            c = V.with_count(consts, n)
            hotpath.cull_indirect_args(c, d_b, d_h, lay, d_args)
            torch.cuda.synchronize()
            want = args0.copy()
            want[:, 11] = V.cull(c, b, hzb, layout)["visible"]
            assert np.array_equal(d_args.cpu().numpy().view(np.uint32).reshape(n, 16), want)
    finally:
        hotpath.set_option(lib.UR_OPT_CULL_STORE, 3)


@pytest.mark.parametrize("n", [200, 1500])
def test_cull_edges_draw_ranges(hotpath, sets, n):
    from tests.test_gpu_cull_draws import _expected, _run
    from unclerenderer_amd.hotpath import to_device
    s = [x for x in sets if x["name"] == "saturate/sponza"][0]
    lay, hzb, layout = _hzb_for(s["levels"])
    b = s["bounds"][np.resize(np.arange(s["bounds"].shape[0]), n)]
    c = V.with_count(s["consts"], n)
    words = V.cull(c, b, hzb, layout)["visible"].astype(np.uint32)
    cmds = _args0(n, n)
    for o in (np.array([0, 0, 1, 1, 2, 2, n // 2, n // 2 + 1, n, n], np.uint32), np.array([0, n], np.uint32), np.arange(n + 1, dtype=np.uint32)):
        got_args, vis, cnt, got_cmds, got_counts = _run(hotpath, c, to_device(b), to_device(hzb), lay, cmds, o)
        want_cmds, want_counts = _expected(words, cmds, o)
        assert np.array_equal(got_args[:, 11], words)
        assert np.array_equal(got_cmds, want_cmds) and np.array_equal(got_counts, want_counts)
        assert cnt == int(words.sum()) and np.array_equal(vis[:cnt], np.flatnonzero(words).astype(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------
# Build HZB on special-value depth buffers
# ---------------------------------------------------------------------------------------------------------------------
def _check_hzb(got, lay, want_levels, what, written=None):
    ok_all = True
    for k, ((o, w, h), (m, free)) in enumerate(zip(lay.as_list(), want_levels)):
        if written is not None and k not in written:
            continue
        g = got[o:o + w * h]
        ok = V.same_bits(g, m.ravel(), free.ravel())
        assert ok.all(), f"{what}: mip {k} ({w}x{h}) differs at {np.flatnonzero(~ok)[:6]}: got {g[~ok][:4]} want {m.ravel()[~ok][:4]}"
        ok_all &= ok.all()
    return ok_all


@pytest.mark.parametrize("w,h", [(17, 9), (129, 67), (640, 360), (1918, 1082), (3840, 2160), (6001, 3999)])
def test_build_hzb_special_depth(hotpath, w, h):
    """One launch plus the tail, two launches and the three-launch sizes (mip 4 too large for the tail's LDS)."""
    from unclerenderer_amd.hotpath import HzbLayout, to_device
    torch = _torch()
    d = V.special_depth(w, h, seed=w)
    lay = HzbLayout(w, h)
    want = V.build_hzb(d)
    hzb = torch.full((lay.total,), float(SENT.view(np.float32)), device="cuda")
    hotpath.build_hzb(to_device(d), hzb, lay)
    torch.cuda.synchronize()
    got = hzb.cpu().numpy()
    _check_hzb(got, lay, want, f"{w}x{h}")
    mask = np.ones(lay.total, bool)
    for (o, mw, mh) in lay.as_list():
        mask[o:o + mw * mh] = False
    assert (got[mask].view(np.uint32) == SENT).all(), "written outside the mips"


@pytest.mark.parametrize("mode", [1, 2])
def test_build_hzb_special_depth_riding_lighting(hotpath, mode):
    """ur_defer_hzb_tail 1 (the tail rides the streaming Lighting launch) and 2 (the whole chain does). The Lighting launch
    reads the ordinary depth buffer; only the HZB is built from the special one."""
    from tests.test_gpu_hzb_tail import _setup
    from unclerenderer_amd.hotpath import to_device
    torch = _torch()
    w, h = 1024, 512
    fc, g, tables, lay, dev = _setup(hotpath, w, h)
    d = V.special_depth(w, h, seed=mode)
    want = V.build_hzb(d)
    dD = to_device(d)
    hotpath.defer_hzb_tail(mode)
    try:
        for it in range(2):
            hzb = torch.full((lay.total,), -1.0, device="cuda")
            hotpath.build_hzb(dD, hzb, lay)
            hotpath.deferred_lighting_sky(fc.scene, fc.sky, dev["A"], dev["B"], dev["C"], dev["D"], tables, to_device(g.hdr), w, h)
            torch.cuda.synchronize()
            _check_hzb(hzb.cpu().numpy(), lay, want, f"mode {mode} launch {it}")
    finally:
        hotpath.defer_hzb_tail(0)


@pytest.mark.parametrize("world", [2, 3])
def test_build_hzb_special_depth_bands(hotpath, world):
    """ur_build_hzb_band per rank, the slices exchanged, then ur_build_hzb_tail: the restatement's chain."""
    from unclerenderer_amd.hotpath import HzbLayout, to_device
    torch = _torch()
    w, h = 1920, 1080
    d = V.special_depth(w, h, seed=10 + world)
    lay = HzbLayout(w, h)
    want = V.build_hzb(d)
    dD = to_device(d)
    whole = torch.full((lay.total,), -1.0, device="cuda")
    for r in range(world):
        p0, pn = lay.band_pieces(world, r)
        mine = torch.full((lay.total,), -1.0, device="cuda")
        hotpath.build_hzb_band(dD, mine, lay, p0, pn)
        torch.cuda.synchronize()
        for off, cnt in lay.band_slices(p0, pn):
            whole[off:off + cnt] = mine[off:off + cnt]
    hotpath.build_hzb_tail(whole, lay)
    torch.cuda.synchronize()
    _check_hzb(whole.cpu().numpy(), lay, want, f"{world} bands")


@pytest.mark.parametrize("w,h", [(640, 360), (1920, 1080)])
def test_cull_against_gpu_built_special_hzb(hotpath, oracle, w, h):
    """The GPU's chain of a special-value depth buffer, read back, is the restatement's; the cull against it (random instances
    and growing boxes about the all-NaN and signed-zero patches) decides as the restatement does."""
    from unclerenderer_amd import hostmath, synth
    from unclerenderer_amd.hotpath import HzbLayout, to_device
    torch = _torch()
    d = V.special_depth(w, h, seed=3)
    lay = HzbLayout(w, h)
    hzb = torch.zeros(lay.total, device="cuda")
    hotpath.build_hzb(to_device(d), hzb, lay)
    torch.cuda.synchronize()
    got = hzb.cpu().numpy()
    _check_hzb(got, lay, V.build_hzb(d), f"{w}x{h}")
    fc = hostmath.build_frame_constants("sponza", w, h)
    n = 20_000
    b = synth.instances_random(n, 8, center=fc.camera_position, box=60.0)
    c = hostmath.pack_culling_constants(fc.view, fc.proj, n, True, lay.count, lay.width, lay.height, True)
    args0 = _args0(n, 4)
    args, stats, vis, cnt = _cull(hotpath, c, b, lay, got, args0)
    want = V.expected_outputs(c, b, got, lay.as_list(), args0)
    assert np.array_equal(args, want[0]) and np.array_equal(stats, want[1]) and cnt == want[3] and np.array_equal(vis[:cnt], want[2])
    assert 0 < want[1][1], "no instance was occluded"
