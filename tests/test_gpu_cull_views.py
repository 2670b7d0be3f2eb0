"""Extra cull views on the GPU (ur_cull_indirect_args_views, ur_frame_set_cull_views): per view a bitmask, an ascending list + count and
draw ranges from the reference's CPU frustum test, in the same launch as the camera's cull.

Expected values come from oracle.cpu_frustum(planes, bounds) (RendererUtils IsAabbInCameraFrustum) and, for ranges, from the _expected
construction of test_gpu_cull_draws.py applied to the view's bits. Every buffer a call must not write is sentinel-filled beforehand and
checked afterwards."""
import numpy as np
import pytest

from tests.test_gpu_cull_draws import SENT, _commands, _expected, _setup

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    return torch


def _u(t):
    return t.cpu().numpy().view(np.uint32)


def _sent(k):
    torch = _torch()
    return torch.full((max(k, 1),), int(SENT.view(np.int32)), dtype=torch.int32, device="cuda")


def _mask_of(bits):
    """uint32[ceil(n / 32)]: bit i & 31 of word i >> 5 = bits[i]."""
    n = bits.size
    w = np.zeros((n + 31) // 32 * 32, np.uint8)
    w[:n] = bits
    return np.packbits(w.reshape(-1, 32)[:, ::-1], axis=1).view(">u4").astype(np.uint32).reshape(-1)


def _view_planes(fc, consts):
    """The four views of the issue: the camera's own planes (plane 4 = (NaN, NaN, NaN, +inf)), the light view enclosing the scene, a
    quarter-radius cascade, a second camera turned 90 degrees."""
    from unclerenderer_amd import hostmath
    cam = np.ascontiguousarray(consts[:24]).view(np.float32).copy()
    light = hostmath.frustum_planes(hostmath.light_view_projection(fc.scene_center, fc.scene_radius, fc.light_direction))
    cascade = hostmath.frustum_planes(hostmath.light_view_projection(fc.scene_center, fc.scene_radius * 0.25, fc.light_direction))
    rot = np.array([[0, 0, -1, 0], [0, 1, 0, 0], [1, 0, 0, 0], [0, 0, 0, 1]], np.float32)  # row-vector convention: v' = v @ rot
    view = np.asarray(fc.view, np.float32).reshape(4, 4)
    turned = hostmath.frustum_planes((view @ rot @ np.asarray(fc.proj, np.float32).reshape(4, 4)).reshape(-1))
    return [cam, light, cascade, turned]


class _View:
    """Sentinel-filled buffers of one view and the call argument that points at them."""

    def __init__(self, planes, n, mask=True, lst=True, offsets=None):
        self.planes, self.n, self.offsets = planes, n, offsets
        words = (n + 31) // 32
        self.mask = _sent(words + 2) if mask else None  # two guard words behind the mask
        self.vis = _sent(n + 1) if lst else None
        self.cnt = _sent(1) if lst else None
        self.cmds = _sent(max(n, 1) * 16) if offsets is not None else None
        self.counts = _sent(offsets.size - 1) if offsets is not None else None
        d = dict(planes=planes)
        if mask:
            d["mask"] = self.mask[:max(words, 1)]
        if lst:
            d.update(visible_idx=self.vis, visible_count=self.cnt)
        if offsets is not None:
            d.update(draw_offsets=offsets, draw_commands=self.cmds, draw_counts=self.counts)
        self.arg = d

    def check(self, oracle, bounds, cmds, index_base=0):
        bits = oracle.cpu_frustum(self.planes, bounds).astype(np.uint8) if self.n else np.zeros(0, np.uint8)
        words = (self.n + 31) // 32
        if self.mask is not None:
            m = _u(self.mask)
            assert np.array_equal(m[:words], _mask_of(bits)), "mask"
            assert (m[words:] == SENT).all(), "mask guard words"
        vis = np.flatnonzero(bits).astype(np.uint32) + np.uint32(index_base)
        if self.vis is not None:
            c = int(_u(self.cnt)[0])
            assert c == vis.size, ("count", c, vis.size)
            got = _u(self.vis)
            assert np.array_equal(got[:c], vis) and (got[c:] == SENT).all(), "list"
        if self.offsets is not None:
            want, want_counts = _expected(bits.astype(np.uint32), cmds, self.offsets)
            assert np.array_equal(_u(self.counts), want_counts), "range counts"
            assert np.array_equal(_u(self.cmds).reshape(-1, 16)[:self.n], want), "range commands"
        return bits


def _camera_call(hotpath, consts, d_bounds, hzb, lay, cmds, views, offsets=None, with_list=True, index_base=0, d_args=None):
    """The camera's call with (or without) views over sentinel outputs; returns the camera's (words, stats, list, count, cmds, counts)."""
    from unclerenderer_amd.hotpath import to_device
    torch = _torch()
    n = cmds.shape[0]
    d_args = to_device(cmds) if d_args is None else d_args
    d_stats = torch.zeros(2, dtype=torch.int32, device="cuda")
    d_vis, d_cnt = (_sent(n), _sent(1)) if with_list else (None, None)
    kw = {}
    if offsets is not None:
        kw = dict(draw_offsets=offsets, draw_commands=_sent(n * 16), draw_counts=_sent(offsets.size - 1))
    hotpath.cull_indirect_args(consts, d_bounds, hzb, lay, d_args, d_stats, d_vis, d_cnt, index_base, views=views, **kw)
    torch.cuda.synchronize()
    return (_u(d_args).reshape(n, 16).copy(), _u(d_stats), _u(d_vis) if with_list else None, int(_u(d_cnt)[0]) if with_list else None,
            _u(kw["draw_commands"]) if kw else None, _u(kw["draw_counts"]) if kw else None)


def _same(a, b):
    for x, y in zip(a, b):
        assert (x is None and y is None) or np.array_equal(x, y)


SIZES = [0, 1, 63, 64, 255, 256, 257, 16383, 16384, 16385, 70_000]


@pytest.mark.parametrize("n", SIZES)
def test_views_match_the_oracle(hotpath, oracle, n):
    from unclerenderer_amd import hostmath
    from unclerenderer_amd.hotpath import to_device
    fc, lay, hzb, bounds = _setup(oracle, max(n, 1), seed=200 + n)
    bounds = bounds[:n]
    consts = hostmath.pack_culling_constants(fc.view, fc.proj, n, True, lay.count, lay.width, lay.height, True)
    cmds = _commands(n, seed=n)
    planes = _view_planes(fc, consts)
    d_bounds, d_hzb = to_device(bounds if n else np.zeros((2, 4), np.float32)), to_device(hzb)
    rng = np.random.default_rng(n)
    layouts = [np.array([0, n], np.uint32), np.linspace(0, n, 65).astype(np.uint32),
               np.sort(np.concatenate([[0], rng.integers(0, n + 1, 4095), [n]])).astype(np.uint32)]
    plain = _camera_call(hotpath, consts, d_bounds, d_hzb, lay, cmds, None)
    for k in (1, 2, 4):
        vs = [_View(planes[i], n, mask=True, lst=(i % 2 == 0) or k == 1, offsets=layouts[(i + k) % 3] if i != 1 else None) for i in range(k)]
        got = _camera_call(hotpath, consts, d_bounds, d_hzb, lay, cmds, [v.arg for v in vs])
        _same(plain[:2], got[:2])
        assert plain[3] == got[3] and np.array_equal(plain[2], got[2])
        for v in vs:
            v.check(oracle, bounds, cmds)
    if n >= 1000:
        assert 0 < oracle.cpu_frustum(planes[2], bounds).sum() < oracle.cpu_frustum(planes[1], bounds).sum(), "the cascade culls"


def test_c5_one_million(hotpath, oracle):
    from unclerenderer_amd import hostmath
    from unclerenderer_amd.hotpath import to_device
    n = 1_000_000
    fc, lay, hzb, bounds = _setup(oracle, n, seed=5, box=400.0, w=960, h=540)
    consts = hostmath.pack_culling_constants(fc.view, fc.proj, n, True, lay.count, lay.width, lay.height, True)
    cmds = _commands(n, seed=5)
    planes = _view_planes(fc, consts)
    d_bounds, d_hzb = to_device(bounds), to_device(hzb)
    ref_args, _, ref_vis, ref_cnt = oracle.cull_indirect_args(consts, bounds, hzb, lay.as_list(), cmds)
    o = np.sort(np.concatenate([[0], np.random.default_rng(4096).integers(0, n + 1, 4095), [n]])).astype(np.uint32)
    vs = [_View(planes[0], n, offsets=o), _View(planes[1], n), _View(planes[2], n, lst=False), _View(planes[3], n, offsets=np.array([0, n], np.uint32))]
    got = _camera_call(hotpath, consts, d_bounds, d_hzb, lay, cmds, [v.arg for v in vs])
    assert np.array_equal(got[0], ref_args) and got[3] == ref_cnt and np.array_equal(got[2][:ref_cnt], ref_vis)
    for v in vs:
        v.check(oracle, bounds, cmds)


@pytest.mark.parametrize("n", [200, 70_000])
def test_camera_outputs_are_unchanged_under_every_store_flavour(hotpath, oracle, n):
    from unclerenderer_amd import hostmath, lib
    from unclerenderer_amd.hotpath import to_device
    fc, lay, hzb, bounds = _setup(oracle, n, seed=300 + n)
    consts = hostmath.pack_culling_constants(fc.view, fc.proj, n, True, lay.count, lay.width, lay.height, True)
    cmds = _commands(n, seed=7)
    ref_args, _, _, _ = oracle.cull_indirect_args(consts, bounds, hzb, lay.as_list(), cmds)
    d_bounds, d_hzb = to_device(bounds), to_device(hzb)
    planes = _view_planes(fc, consts)
    o = np.linspace(0, n, 9).astype(np.uint32)
    garbage = cmds.copy()
    garbage[:, 11] = np.random.default_rng(1).integers(0, 2 ** 32, n, dtype=np.uint32)
    starts = {"zeros": 0, "ones": 1, "oracle": None, "garbage": None}
    old = hotpath.get_option(lib.UR_OPT_CULL_STORE)
    try:
        for flavour in (0, 1, 2, 3, 4):
            hotpath.set_option(lib.UR_OPT_CULL_STORE, flavour)
            for name in starts:
                start = cmds.copy()
                if name in ("zeros", "ones"):
                    start[:, 11] = starts[name]
                elif name == "oracle":
                    start = ref_args.copy()
                else:
                    start = garbage
                a = to_device(start)
                b = to_device(start)
                plain = _camera_call(hotpath, consts, d_bounds, d_hzb, lay, cmds, None, offsets=o, d_args=a)
                vs = [_View(planes[i], n, offsets=o) for i in range(4)]
                got = _camera_call(hotpath, consts, d_bounds, d_hzb, lay, cmds, [v.arg for v in vs], offsets=o, d_args=b)
                _same(plain, got)
                assert np.array_equal(got[0], ref_args), (flavour, name)
                for v in vs:
                    v.check(oracle, bounds, cmds)
                if flavour == 4:  # the record is the camera's: a view-less call on the same buffer still gives the oracle's words
                    again = _camera_call(hotpath, consts, d_bounds, d_hzb, lay, cmds, None, d_args=b)
                    assert np.array_equal(again[0], ref_args), name
    finally:
        hotpath.set_option(lib.UR_OPT_CULL_STORE, old)


def _fma_flip_pair(rng):
    """A plane and a p-vertex whose d is >= 0 summed in float32 without contraction but < 0 when the first product is fused into the
    second sum (fma(x, X, y*Y) rounded once), found on the host."""
    f = np.float32
    for _ in range(200000):
        P = rng.standard_normal(4).astype(f)
        V = rng.standard_normal(3).astype(f) * f(10)
        xy = f(f(P[0] * V[0]) + f(P[1] * V[1]))
        z = f(P[2] * V[2])
        w = f(-(float(xy) + float(z)))  # w near -(xy + z): d close to 0
        d = f(f(xy + z) + w)
        fused = f(float(P[0]) * float(V[0]) + float(f(P[1] * V[1])))  # float64 product and sum, one rounding: np.fma-style
        dfma = f(f(fused + z) + w)
        if (d >= 0) != (dfma >= 0):
            return np.array([P[0], P[1], P[2], w], f), V
    return None, None


def _edge_set(planes_list, rng):
    """AABBs whose p-vertex puts d at 0, the adjacent floats either side, +-0 and +-denormal for each plane of each frustum; plus
    plane components of -0 and NaN, NaN and +-inf bounds, and the fma pair."""
    f = np.float32
    boxes = []
    for planes in planes_list:
        P6 = planes.reshape(6, 4)
        for i in range(6):
            P = P6[i]
            if not np.isfinite(P).all() or not P[:3].any():
                continue
            for target in (f(0), f(-0.0), np.nextafter(f(0), f(1)), np.nextafter(f(0), f(-1)), f(1e-42), f(-1e-42)):
                for _ in range(4):
                    V = (rng.standard_normal(3) * 20).astype(f)
                    # solve on the axis with the largest |P| for d == target, then walk to the float that lands exactly
                    k = int(np.argmax(np.abs(P[:3])))
                    rest = sum(float(P[j]) * float(V[j]) for j in range(3) if j != k) + float(P[3])
                    V[k] = f((float(target) - rest) / float(P[k]))
                    for _it in range(64):
                        d = f(f(f(f(P[0] * V[0]) + f(P[1] * V[1])) + f(P[2] * V[2])) + f(P[3] * f(1)))
                        if d == target:
                            break
                        V[k] = np.nextafter(V[k], f(np.inf) if (d < target) == (P[k] > 0) else f(-np.inf))
                    lo = np.where(P[:3] >= 0, V - f(5), V)
                    hi = np.where(P[:3] >= 0, V, V + f(5))
                    boxes.append((lo, hi))
    specials = [np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-42]
    for a in specials:
        for axis in range(3):
            lo, hi = np.full(3, -1, f), np.full(3, 1, f)
            lo[axis] = f(a)
            boxes.append((lo.copy(), hi.copy()))
            hi[axis] = f(a)
            boxes.append((np.full(3, -1, f), hi))
    b = np.zeros((len(boxes), 2, 4), f)
    for j, (lo, hi) in enumerate(boxes):
        b[j, 0, :3], b[j, 1, :3] = lo, hi
    return b


def test_decision_edges(hotpath, oracle):
    from unclerenderer_amd import hostmath
    from unclerenderer_amd.hotpath import to_device
    fc, lay, hzb, _ = _setup(oracle, 1, seed=1)
    consts0 = hostmath.pack_culling_constants(fc.view, fc.proj, 1, False, 0, 0, 0, True)
    planes = _view_planes(fc, consts0)
    rng = np.random.default_rng(12)
    P, V = _fma_flip_pair(rng)
    assert P is not None, "no fma-flip pair found"
    fma_planes = np.tile(np.array([0, 0, 0, 1], np.float32), 6)
    fma_planes[:4] = P
    odd = planes[1].copy()
    odd[0] = -0.0  # a -0 component picks max
    odd[5] = np.nan  # a NaN component picks min
    odd[9] = -0.0
    bounds = _edge_set([planes[0], planes[1], odd], rng).reshape(-1, 4)
    fb = np.zeros((2, 4), np.float32)
    fb[0, :3] = np.where(P[:3] >= 0, V - 1, V)
    fb[1, :3] = np.where(P[:3] >= 0, V, V + 1)
    bounds = np.concatenate([bounds, fb]).astype(np.float32)
    n = bounds.shape[0] // 2
    consts = hostmath.pack_culling_constants(fc.view, fc.proj, n, False, 0, 0, 0, True)
    cmds = _commands(n, seed=3)
    d_bounds = to_device(bounds)
    for group in ([planes[0], planes[1], odd, fma_planes],):
        vs = [_View(p, n) for p in group]
        _camera_call(hotpath, consts, d_bounds, None, None, cmds, [v.arg for v in vs])
        bits = [v.check(oracle, bounds.reshape(-1, 2, 4), cmds) for v in vs]
    # the fma pair is decided as the unfused sum decides it
    assert bits[3][-1] == oracle.cpu_frustum(fma_planes, fb)[0]
    # both sides of the edges occur
    for b in bits[:3]:
        assert 0 < b.sum() < n


@pytest.mark.parametrize("ranks", [2, 3])
def test_instance_range_sharding(hotpath, oracle, ranks):
    from unclerenderer_amd import hostmath
    from unclerenderer_amd.hotpath import to_device
    n = 70_001
    fc, lay, hzb, bounds = _setup(oracle, n, seed=77)
    planes = _view_planes(fc, hostmath.pack_culling_constants(fc.view, fc.proj, n, False, 0, 0, 0, True))[1:3]
    cmds = _commands(n, seed=77)
    whole = [_View(p, n) for p in planes]
    consts = hostmath.pack_culling_constants(fc.view, fc.proj, n, True, lay.count, lay.width, lay.height, True)
    _camera_call(hotpath, consts, to_device(bounds), to_device(hzb), lay, cmds, [v.arg for v in whole])
    cut = np.linspace(0, n, ranks + 1).astype(np.int64)
    lists = [[] for _ in planes]
    for r in range(ranks):
        a, b = int(cut[r]), int(cut[r + 1])
        c = hostmath.pack_culling_constants(fc.view, fc.proj, b - a, True, lay.count, lay.width, lay.height, True)
        part = [_View(p, b - a) for p in planes]
        _camera_call(hotpath, c, to_device(bounds[a:b]), to_device(hzb), lay, cmds[a:b], [v.arg for v in part], index_base=a)
        for k, v in enumerate(part):
            v.check(oracle, bounds[a:b], cmds[a:b], index_base=a)
            lists[k].append(_u(v.vis)[:int(_u(v.cnt)[0])])
    for k, v in enumerate(whole):
        assert np.array_equal(np.concatenate(lists[k]), _u(v.vis)[:int(_u(v.cnt)[0])])


def test_a_workspace_with_no_slack(hotpath, oracle):
    """The workspace grown inside the call, so that it has no slack: a view's slice that overran its neighbour would land in the next
    slice, not in spare room. ur_create reserves 1 << 20 instances, so the sizes lie just above that, on a context of its own:
    n = (1 << 20) + 1 makes the call itself reserve 4097 * 256 instances: 4097 blocks in a stride of 4097, every slice exactly full, 65
    compaction workgroups per row; the same call again on the same command buffer meets a valid record (flavour 4) on that exact
    workspace; n = (1 << 20) + 16385 grows it again inside the call (4161 blocks, stride 4161) and drops the record; and that call again.
    Four views, all compacted, two with lists and two with ranges; the camera with a list and ranges; UR_OPT_CULL_STORE = 4. Every call's
    words, lists, counts and range commands are the oracle's (one oracle run at the larger n: an instance's result does not depend on n)."""
    from unclerenderer_amd import hostmath, lib
    from unclerenderer_amd.hotpath import HotPath, to_device
    n_max = (1 << 20) + 16385
    fc, lay, hzb, all_bounds = _setup(oracle, n_max, seed=901, box=400.0, w=960, h=540)
    all_cmds = _commands(n_max, seed=902)
    consts_of = lambda n: hostmath.pack_culling_constants(fc.view, fc.proj, n, True, lay.count, lay.width, lay.height, True)
    all_args, _, all_vis, _ = oracle.cull_indirect_args(consts_of(n_max), all_bounds, hzb, lay.as_list(), all_cmds)
    planes = _view_planes(fc, consts_of(n_max))
    d_bounds, d_hzb = to_device(all_bounds), to_device(hzb)
    own = HotPath(0)
    try:
        own.set_option(lib.UR_OPT_CULL_STORE, 4)
        for n in ((1 << 20) + 1, n_max):
            consts, bounds, cmds = consts_of(n), all_bounds[:n], all_cmds[:n]
            ref_args, ref_vis = all_args[:n], all_vis[all_vis < n]
            d_args = to_device(cmds)
            o = np.linspace(0, n, 9).astype(np.uint32)
            want_cmds, want_counts = _expected(ref_args[:, 11], cmds, o)
            for call in (1, 2):  # (the first grows the workspace inside the call; the second meets the record the first left)
                vs = [_View(planes[0], n), _View(planes[1], n, lst=False, offsets=o), _View(planes[2], n),
                      _View(planes[3], n, lst=False, offsets=np.array([0, n // 3, n], np.uint32))]
                got = _camera_call(own, consts, d_bounds[:n], d_hzb, lay, cmds, [v.arg for v in vs], offsets=o, d_args=d_args)
                assert np.array_equal(got[0], ref_args), (n, call, "words")
                assert got[3] == ref_vis.size and np.array_equal(got[2][:got[3]], ref_vis) and (got[2][got[3]:] == SENT).all(), (n, call, "list")
                assert np.array_equal(got[5], want_counts) and np.array_equal(got[4].reshape(-1, 16)[:n], want_cmds), (n, call, "ranges")
                for v in vs:
                    v.check(oracle, bounds, cmds)
    finally:
        own.close()


# ---------------------------------------------------------------------------------------------------------------------
# The frame
# ---------------------------------------------------------------------------------------------------------------------
def _frame(hotpath, name, bounds, flags, set_views, frames=2, seed=31):
    import torch
    from unclerenderer_amd import hostmath, synth
    from unclerenderer_amd.hotpath import Frame, HzbLayout, to_device
    w, h, n = 128, 72, bounds.shape[0]
    fc = hostmath.build_frame_constants(name, w, h, shadow_size=128, env_mip_count=5)
    g = synth.gbuffer_scene(fc.view, fc.proj, fc.camera_position, w, h, seed)
    shadow, env, lut = synth.shadow_map_noise(128, seed), synth.env_cube_procedural(16, 5), synth.brdf_lut_procedural(64, 16)
    tables = hotpath.make_tables(to_device(shadow), hotpath.stage_env_cube(env, 16, 5), 16, 5, to_device(lut))
    lay = HzbLayout(w, h)
    cmds = _commands(n, seed)
    dA, dB, dC, dD = to_device(g.A), to_device(g.B), to_device(g.C), to_device(g.depth)
    d_hzb = torch.zeros(lay.total, device="cuda")
    d_bounds, d_args, d_stats = to_device(bounds), to_device(cmds), torch.zeros(2, dtype=torch.int32, device="cuda")
    d_vis, d_cnt = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    consts = hostmath.pack_culling_constants(fc.view, fc.proj, 0, False, 0, 0, 0, True)
    full = hostmath.pack_culling_constants(fc.view, fc.proj, n, False, 0, 0, 0, True)
    planes = _view_planes(fc, full)
    views = [_View(planes[0], n, offsets=np.array([0, n // 3, n], np.uint32)), _View(planes[1], n)]
    frame = Frame(hotpath)
    if set_views:
        frame.set_cull_views([v.arg for v in views])
    out = []
    for _ in range(frames):
        d_args.copy_(to_device(cmds))
        hdr = to_device(g.hdr)
        res = Frame.resources(w, h, 0, h, dA, dB, dC, dD, hdr, dD, d_hzb, lay, tables, d_bounds, d_args, n, 0, d_vis, d_cnt, d_stats)
        frame.render(res, consts, fc.scene, fc.sky, flags)
        torch.cuda.synchronize()
        out.append((_u(d_args).reshape(n, 16).copy(), _u(d_vis).copy(), int(_u(d_cnt)[0]), _u(hdr).copy(), frame.report()))
    frame.close()
    return cmds, views, out


def _check_frame(hotpath, oracle, name, bounds, flags):
    from unclerenderer_amd import lib
    cmds, _, plain = _frame(hotpath, name, bounds, flags, set_views=False)
    _, views, got = _frame(hotpath, name, bounds, flags | lib.UR_FRAME_CULL_VIEWS, set_views=True)
    for p, g in zip(plain, got):
        assert np.array_equal(p[0], g[0]) and p[2] == g[2] and np.array_equal(p[1][:p[2]], g[1][:g[2]])
        assert np.array_equal(p[3], g[3]), "the HDR bytes are the same with views"
        assert p[4] == g[4], "the pass list is the same with views"
    for v in views:
        v.check(oracle, bounds, cmds)
    # views set but no flag: their buffers stay sentinel, the frame is the plain one
    _, idle, off = _frame(hotpath, name, bounds, flags, set_views=True, frames=1)
    for v in idle:
        for t in (v.mask, v.vis, v.cnt, v.cmds, v.counts):
            assert t is None or (_u(t) == SENT).all()
    assert np.array_equal(off[0][3], plain[0][3]) and np.array_equal(off[0][0], plain[0][0])


@pytest.mark.parametrize("async_compute", [False, True])
def test_frame_pica_pica(hotpath, oracle, async_compute):
    from pathlib import Path
    from unclerenderer_amd import lib, scene
    sb = scene.load_scene_bounds(Path(__file__).parent / "golden" / "assets" / "Scenes" / "pica_pica.json")
    _check_frame(hotpath, oracle, "pica_pica", sb.bounds, lib.UR_FRAME_DEFAULT | (lib.UR_FRAME_ASYNC_COMPUTE if async_compute else 0))


@pytest.mark.parametrize("async_compute", [False, True])
def test_frame_synthetic_4097(hotpath, oracle, async_compute):
    from unclerenderer_amd import hostmath, lib, synth
    fc = hostmath.build_frame_constants("sponza", 128, 72)
    bounds = synth.instances_random(4097, 33, center=fc.camera_position, box=60.0)
    _check_frame(hotpath, oracle, "sponza", bounds, lib.UR_FRAME_DEFAULT | (lib.UR_FRAME_ASYNC_COMPUTE if async_compute else 0))


def test_frame_disabled_cull_leaves_views_alone(hotpath, oracle):
    from unclerenderer_amd import hostmath, lib, synth
    fc = hostmath.build_frame_constants("sponza", 128, 72)
    bounds = synth.instances_random(300, 35, center=fc.camera_position, box=60.0)
    _, views, out = _frame(hotpath, "sponza", bounds, (lib.UR_FRAME_DEFAULT & ~lib.UR_FRAME_INDIRECT_DRAW) | lib.UR_FRAME_CULL_VIEWS,
                           set_views=True, frames=1)
    for v in views:
        for t in (v.mask, v.vis, v.cnt, v.cmds, v.counts):
            assert t is None or (_u(t) == SENT).all()
    assert out[0][4][0][0] == "GPU Culling"
