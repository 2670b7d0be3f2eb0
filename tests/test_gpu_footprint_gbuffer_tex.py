"""Footprint rules (tests/footprint.py, run_rules unchanged) for ur_gbuffer_pass_materials: beside what tests/test_gpu_footprint_gbuffer.py
guards - the band targets, the key scratch, the stats, depth, the command slots and the buffers they point at - every texture's packed
levels and the material table are touched only where include/ur_raster.h says: read inside, never written, nothing around them.

The command slots and the material table hold the addresses of the guarded buffers of their run, so they are packed inside the call and
guarded here by hand with the run's poison; their guards and payload are checked when the runs are over."""
import numpy as np
import pytest

from tests import depth_ref as D
from tests import footprint as fp
from tests import gbuffer_tex_ref as X

pytestmark = pytest.mark.gpu


def _guarded_run(hotpath, draws, mats, view, proj, w, h, band, reserve, flags, what):
    """fp.run_rules on one ur_gbuffer_pass_materials call with every buffer guarded, the command slots and the material table by hand;
    a map a material does not have stays a zero descriptor. Returns (the plain run's outputs, the depth the call was given)."""
    import torch
    from unclerenderer_amd import lib
    from unclerenderer_amd.hotpath import gbuffer_targets, pack_draw_commands
    row0, rows = band
    depth, _ = D.depth_prepass(draws, view, proj, w, h, flags=flags)
    inputs = {"depth": depth}
    for k, d in enumerate(draws):
        inputs[f"vertices{k}"] = np.ascontiguousarray(d.vertices).view(np.uint8)
        inputs[f"indices{k}"] = np.ascontiguousarray(d.indices, np.uint32)
        inputs[f"constants{k}"] = d.constants()
        for name, _, _ in X.MAPS:
            if mats[k].get(name) is not None:
                inputs[f"texture{k}_{name}"] = np.concatenate([a.reshape(-1) for a in mats[k][name].levels]).view(np.uint32)
    half = np.full((rows, w, 4), np.nan, np.float16)
    word = np.full((rows, w), 0x5A5A5A5A, np.uint32)
    outputs = {"A": half, "B": half.copy(), "hdr": half.copy(), "C": word, "keys": word.copy(), "object_id": word.copy(),
               "stats": np.array([5, 6, 7, 8, 9, 10], np.uint32)}
    held = []

    def by_hand(host, like):
        poison = getattr(like, "footprint", None)
        dev = fp.guarded(host, "cuda", poison.fill) if poison is not None else fp.plain(host, "cuda")
        held.append((dev, host))
        return dev

    def call(b):
        spec = [dict(vertices=b[f"vertices{k}"], indices=b[f"indices{k}"], constants=b[f"constants{k}"], stride=d.stride, index_count=d.count(),
                     start_index=d.start_index, base_vertex=d.base_vertex) for k, d in enumerate(draws)]
        cmds = by_hand(pack_draw_commands(spec), b["depth"])
        rec = (lib.Material * len(mats))()
        for k, m in enumerate(mats):
            rec[k].pipeline_key = m["key"]
            for name, _, _ in X.MAPS:
                t = m.get(name)
                if t is None:
                    continue
                setattr(rec[k], name, lib.Texture2D(b[f"texture{k}_{name}"].data_ptr(), t.width, t.height, len(t.levels),
                                                    lib.UR_TEXTURE_R8G8B8A8_UNORM_SRGB if t.srgb else lib.UR_TEXTURE_R8G8B8A8_UNORM, 0))
        table = by_hand(np.frombuffer(bytes(rec), np.uint32).copy(), b["depth"])
        tg = gbuffer_targets(b["A"], b["B"], b["C"], b["hdr"], b["keys"], b["object_id"])
        hotpath.gbuffer_pass(view, proj, cmds, b["depth"], tg, w, h, row0, rows, stats=b["stats"], flags=flags, materials=(table, len(mats)))

    hotpath.raster_reserve(reserve)
    try:
        got = fp.run_rules(call, inputs, outputs, what=f"ur_gbuffer_pass_materials, {what}, reserve {reserve}, flags {flags}, rows {band}")
    finally:
        torch.cuda.synchronize()
        hotpath.raster_reserve(0)
    for dev, host in held:
        if hasattr(dev, "footprint"):
            r = fp.check(dev)
            assert r.ok, f"command slots / material table: {r}"
        assert np.array_equal(fp.host_bytes(dev), host.view(np.uint8).reshape(-1)), "the command slots or the material table were written"
    return got, depth


@pytest.mark.parametrize("reserve,flags,band", [(4096, 0, (37, 41)), (0, X.G.QUANTIZE_D24, (0, 130))])
def test_gbuffer_pass_materials_footprint(hotpath, reserve, flags, band):
    w, h = 257, 130  # off every tile and stamp multiple
    row0, rows = band
    draws = X.soup(w, h, 11, triangles=500)
    mats = X.soup_materials(11)
    view, proj = D.soup_camera(w, h)
    got, depth = _guarded_run(hotpath, draws, mats, view, proj, w, h, band, reserve, flags, "soup")
    want = X.gbuffer_pass(draws, view, proj, depth, w, h, materials=mats, flags=flags)
    assert set(want["shade32"]["bits"][(want["gather"]["py"] >= row0) & (want["gather"]["py"] < row0 + rows)].tolist()) >= {1, 2, 4, 15}
    for k in ("keys", "C", "object_id"):
        assert np.array_equal(got[k], want[k][row0:row0 + rows]), k
    for k in ("A", "B", "hdr"):
        g, e = got[k].view(np.uint16), want[k][row0:row0 + rows]
        nan = np.isnan(got[k])
        assert np.array_equal(nan, np.isnan(e.view(np.float16))) and np.array_equal(g[~nan], e[~nan]), k
    delta = got["stats"] - np.array([5, 6, 7, 8, 9, 10], np.uint32)
    assert delta[[0, 1, 2, 4, 5]].tolist() == want["stats"][[0, 1, 2, 4, 5]].tolist()


RANGE_END_CASES = ["nan_u_one_level", "nan_u_four_levels", "inf_v", "nan_uv", "limit_kept_positive", "limit_dropped_positive", "limit_kept_negative",
                   "limit_dropped_negative", "chain33_nan", "chain33_gradient_2p30", "chain255_nan", "chain255_gradient_2p30"]


def test_coordinates_and_chains_at_the_ends_of_their_ranges_stay_inside_the_texture(hotpath):
    """The hand cases of tests/test_gbuffer_tex_ref.py whose coordinate is not finite or lies at the 2^30 limit, and the 33- and 255-level
    chains (the last level by a NaN, levels 32 and 33 by a finite gradient): the gather stays inside the texture's packed levels - the
    guards around it are never read (the outputs do not depend on their fill) - and the result is the restatement's."""
    from tests.test_gbuffer_tex_ref import H, W, hand_cases
    cases = hand_cases()
    cam = D.hand_camera(W, H)
    for name in RANGE_END_CASES:
        draws, mats = cases[name]
        got, depth = _guarded_run(hotpath, draws, mats, *cam, W, H, (0, H), 0, 0, name)
        want = X.gbuffer_pass(draws, *cam, depth, W, H, materials=mats)
        for k in ("keys", "C", "object_id", "hdr"):
            assert np.array_equal(got[k].view(want[k].dtype), want[k]), (name, k)
