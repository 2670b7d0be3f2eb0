"""UR_FRAME_DEBUG_PRINT on the MI355X: the "GpuDebugPrint" pass is the last live pass and prints the counters the oracle's cull gives
for the same inputs; a frame without the flag is byte for byte the frame it was; row bands through the post exchange equal the
unsplit frame once the ranks' counters are summed."""
import numpy as np
import pytest

from tests import debug_print_ref as R

pytestmark = pytest.mark.gpu

W, H = 1920, 1080
BASE = ["GPU Culling", "Build HZB", "Lighting", "Sky"]


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _words(t):
    return t.cpu().numpy().view(np.uint32)


class _Font:
    def __init__(self):
        torch = _torch()
        from unclerenderer_amd import hostmath
        from unclerenderer_amd.hotpath import to_device
        self.atlas, self.glyphs, self.first, self.count = hostmath.debug_font()
        self.d_atlas, self.d_glyphs = torch.from_numpy(self.atlas).cuda(), to_device(self.glyphs)


def _band_frame(hotpath, inp, rank, world, font, with_debug=True):
    """tests/_post_band_worker.BandFrame plus cull_stats and, with_debug, the text buffer and font."""
    torch = _torch()
    from tests._post_band_worker import BandFrame
    from unclerenderer_amd.hotpath import debug_print_buffer
    f = BandFrame(hotpath, inp, rank, world)
    f.stats = torch.full((2,), 0x1234, dtype=torch.int32, device="cuda")  # stale values: the frame resets them under the flag
    f.res.cull_stats = f.stats.data_ptr()
    f.buf = debug_print_buffer()
    f.buf.fill_(0x5A5A5A5A)
    if with_debug:
        f.frame.set_debug_print(f.buf, font.d_glyphs, font.d_atlas, font.first, font.count)
    return f


def _render(f, post, exchange, debug, extra=0):
    from unclerenderer_amd import lib
    f.frame.set_post(luminance=f.lum, tonemap_scratch=f.scratch, delta_time=1 / 60)
    f.hdr.copy_(f.inp.hdr0[f.plan.row0:f.plan.row0 + f.plan.rows])
    f.args.copy_(f.args0)
    flags = lib.UR_FRAME_DEFAULT | lib.UR_FRAME_FUSE_LIGHTING_SKY | lib.UR_FRAME_TONEMAP | post | extra
    if exchange:
        flags |= lib.UR_FRAME_POST_EXCHANGE
    if debug:
        flags |= lib.UR_FRAME_DEBUG_PRINT
    f.frame.render(f.res, f.consts, f.inp.fc.scene, f.inp.fc.sky, flags)


def _expected_entries(frustum, occluded):
    ref = R.Buffer()
    R.print_stats(ref, int(frustum), int(occluded))
    return ref


@pytest.mark.parametrize("spec", ["", "CAS", "AE|CAS|FUSE"])
def test_last_pass_prints_the_oracles_counters(hotpath, oracle, spec):
    torch = _torch()
    from tests._post_band_worker import Inputs, post_flags
    from unclerenderer_amd import lib
    from unclerenderer_amd.hotpath import HzbLayout
    font, inp = _Font(), Inputs(hotpath, W, H)
    f = _band_frame(hotpath, inp, 0, 1, font)
    plain = _band_frame(hotpath, inp, 0, 1, font, with_debug=False)
    post = post_flags(spec) if spec else 0
    lay = HzbLayout(W, H)
    n = inp.bounds.shape[0]
    args0 = _words(f.args0).reshape(n, 16)
    for k in range(2):  # the first cull has no HZB, the second reads the first frame's
        hzb_before = f.hzb.cpu().numpy().copy()
        _render(f, post, False, True)
        _render(plain, post, False, False)
        torch.cuda.synchronize()
        names = f.frame.report()
        live = [r[0] for r in names if not r[1]]
        assert live[-1] == "GpuDebugPrint" and [r[0] for r in names][-1] == "GpuDebugPrint"
        # the flagless frame's passes and transitions, except: "GPU Culling" also writes the counters and the buffer. The buffer stays in
        # UNORDERED_ACCESS; the counters come back from the last pass's read state from the second frame on (one transition), and the
        # last pass takes them to its read state every frame (one transition; the buffer and the back buffer are in its states already)
        want = [(r[0], r[1], r[2] + (k if r[0] == "GPU Culling" else 0)) for r in plain.frame.report()] + [("GpuDebugPrint", False, 1)]
        assert names == want, (k, names, want)
        c = f.consts.copy()
        c[41], c[45] = (1 if k else 0), 1
        _, ref_stats, _, _ = oracle.cull_indirect_args(c, inp.bounds, hzb_before if k else None, lay.as_list(), args0)
        got_stats = _words(f.stats)
        assert np.array_equal(got_stats, ref_stats), (k, got_stats, ref_stats)
        if k:
            assert ref_stats[1] > 0 or ref_stats[0] > 0
        ref = _expected_entries(ref_stats[0], ref_stats[1])
        got = _words(f.buf)
        assert int(got[0]) == ref.count and np.array_equal(got[1:1 + 4 * ref.count], ref.words()[1:1 + 4 * ref.count])
        # the picture: the flagless frame's bytes with the two lines composited by the restatement (opaque white on texel centres: exact)
        base = R.unpack_rgba(_words(plain.ldr))
        want, lo, hi, cov = R.composite(base, ref, font.glyphs, font.atlas, font.first, font.count)
        assert (lo == hi).all() and cov.sum() == 64 * ref.count
        assert np.array_equal(R.unpack_rgba(_words(f.ldr)), want)
        assert torch.equal(f.hdr, plain.hdr) and torch.equal(f.args, plain.args)
    for x in (f, plain):
        x.close()


def test_without_the_flag_nothing_changes(hotpath):
    torch = _torch()
    from tests._post_band_worker import Inputs, post_flags
    font, inp = _Font(), Inputs(hotpath, W, H)
    before = _band_frame(hotpath, inp, 0, 1, font, with_debug=False)   # a frame that never heard of the call
    after = _band_frame(hotpath, inp, 0, 1, font, with_debug=True)     # the resources are set, the flag is not
    for spec in ("", "AE|CAS", "CAS|FUSE"):
        post = post_flags(spec) if spec else 0
        for x in (before, after):
            x.stats.fill_(0x1234)
            _render(x, post, False, False)
        torch.cuda.synchronize()
        assert before.frame.report() == after.frame.report() and "GpuDebugPrint" not in [r[0] for r in after.frame.report()]
        assert before.frame.report_async() == after.frame.report_async()
        for a, b in ((before.ldr, after.ldr), (before.hdr, after.hdr), (before.args, after.args), (before.hzb, after.hzb), (before.vis, after.vis),
                     (before.cnt, after.cnt), (before.stats, after.stats)):
            assert torch.equal(a, b), spec
        assert _words(after.stats).tolist() == [0x1234, 0x1234]          # dword 45 stays the caller's: nothing counted, nothing reset
        assert (_words(after.buf) == 0x5A5A5A5A).all()                    # the buffer is not touched
    for x in (before, after):
        x.close()


def test_flag_without_resources_is_einval(hotpath):
    torch = _torch()
    from tests._post_band_worker import Inputs
    from unclerenderer_amd import lib
    font, inp = _Font(), Inputs(hotpath, W, H)
    f = _band_frame(hotpath, inp, 0, 1, font, with_debug=False)
    with pytest.raises(lib.UrError) as e:
        _render(f, 0, False, True)                                  # no buffer / font
    assert e.value.code == lib.UR_EINVAL
    f.frame.set_debug_print(f.buf, font.d_glyphs, font.d_atlas, font.first, font.count)
    f.res.cull_stats = None
    with pytest.raises(lib.UrError) as e:
        _render(f, 0, False, True)                                  # no cull_stats
    assert e.value.code == lib.UR_EINVAL
    f.res.cull_stats = f.stats.data_ptr()
    f.res.tonemap_band = None
    with pytest.raises(lib.UrError) as e:
        _render(f, 0, False, True)                                  # no tonemap_band
    assert e.value.code == lib.UR_EINVAL
    f.res.tonemap_band = f.ldr.data_ptr()
    with pytest.raises(lib.UrError) as e:
        f.frame.render(f.res, f.consts, inp.fc.scene, inp.fc.sky, lib.UR_FRAME_DEFAULT | lib.UR_FRAME_DEBUG_PRINT)  # no TONEMAP
    assert e.value.code == lib.UR_EINVAL
    _render(f, 0, False, True)                                      # and with everything it renders
    torch.cuda.synchronize()
    assert f.frame.report()[-1][0] == "GpuDebugPrint"
    f.close()


def test_async_compute_lane_waits_for_the_cull(hotpath):
    torch = _torch()
    from tests._post_band_worker import Inputs
    from unclerenderer_amd import lib
    font, inp = _Font(), Inputs(hotpath, W, H)
    f, g = _band_frame(hotpath, inp, 0, 1, font), _band_frame(hotpath, inp, 0, 1, font)
    for _ in range(2):
        _render(f, 0, False, True)
        _render(g, 0, False, True, extra=lib.UR_FRAME_ASYNC_COMPUTE)
        torch.cuda.synchronize()
        rep = {r[0]: r for r in g.frame.report_async()}
        assert rep["GPU Culling"][1] and not rep["GpuDebugPrint"][1] and rep["GpuDebugPrint"][2] >= 1  # a cross-stream wait on the cull's outputs
        assert torch.equal(f.ldr, g.ldr) and torch.equal(f.stats, g.stats) and torch.equal(f.buf, g.buf)
    for x in (f, g):
        x.close()


@pytest.mark.parametrize("world", [2, 3])
def test_bands_through_the_post_exchange(hotpath, world):
    """Virtual ranks: each band's cull counts its own instance range; with the counters summed over the ranks (what
    dist.allreduce_cull_stats does between processes) every band prints the totals and the bands are the unsplit frame's bytes."""
    torch = _torch()
    from tests._post_band_worker import Inputs, post_flags
    font, inp = _Font(), Inputs(hotpath, W, H)
    ref = _band_frame(hotpath, inp, 0, 1, font)
    bands = [_band_frame(hotpath, inp, r, world, font) for r in range(world)]
    for k, spec in enumerate(("AE|CAS", "CAS|FUSE", "AE|CAS")):
        post = post_flags(spec)
        _render(ref, post, False, True)
        for f in bands:
            _render(f, post, True, True)
            assert [r[0] for r in f.frame.report()] == BASE + ["Post Record"]
        torch.cuda.synchronize()
        allrec = torch.cat([f.own for f in bands]).view(world, -1)
        total = sum(f.stats.clone() for f in bands)
        for f in bands:
            f.records.copy_(allrec)
            f.stats.copy_(total)          # dist.allreduce_cull_stats
        assert torch.equal(total, ref.stats), (k, total, ref.stats)
        for f in bands:
            f.finish()
        torch.cuda.synchronize()
        assert torch.equal(torch.cat([f.ldr for f in bands]), ref.ldr), spec
        for f in bands:
            assert f.frame.report()[-1][0] == "GpuDebugPrint" and torch.equal(f.buf[:1 + 4 * 26], ref.buf[:1 + 4 * 26])
    for x in [ref] + bands:
        x.close()
