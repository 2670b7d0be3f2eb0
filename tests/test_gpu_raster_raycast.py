"""ur_shadow_map, ur_depth_prepass and ur_gbuffer_pass held directly to the float64 ray caster (tests/raycast_ref.py) on its scenes of
connected meshes: the rules of which texels are compared and how closely are that file's, the same that tests/test_raycast_ref.py
applies to the restatements. GBuffer runs over the depth the prepass wrote in the same stream."""
import numpy as np
import pytest

from tests import depth_ref as D
from tests import gbuffer_ref as G
from tests import raycast_ref as R
from tests import shadow_ref as S
from tests import shadow_gpu
from tests.gbuffer_gpu import device_draws, run
from tests.test_raycast_ref import report

pytestmark = pytest.mark.gpu


def camera_passes(hotpath, sc, draws, w, h):
    """(depth (h, w) float32, gbuffer dict) of the two kernels over the draws, one stream, no synchronisation in between."""
    import torch
    dd = device_draws(draws)
    dev_depth = torch.full((h, w), float("nan"), dtype=torch.float32, device="cuda")
    hotpath.depth_prepass(sc.view, sc.proj, dd.commands, dev_depth)
    got = run(hotpath, dd, sc.view, sc.proj, dev_depth, w, h)
    return dev_depth.cpu().numpy(), got


def held(record_property, what, rc, draws, depth, got):
    res = R.compare_gbuffer(rc, got, draws, G.A_ULPS_BOUND, G.C_CODES_BOUND)
    res["depth"] = R.compare_depth(rc, depth, D.DEPTH_ERROR_BOUND, 0.0)["depth"]
    res["depth covered"] = R.compare_depth(rc, depth, D.DEPTH_ERROR_BOUND, 0.0)["covered"]
    report(record_property, what, res)
    assert R.failures(res) == 0, (what, res)


@pytest.mark.parametrize("w,h", R.TARGETS)
def test_shadow_map(hotpath, record_property, w, h):
    sc, rc = R.cast_scene("shadow", w, h)
    got, stats = shadow_gpu.run(hotpath, device_draws(sc.draws), sc.lvp, w, h)
    assert stats[1] == 0 and stats[2] == 0, stats.tolist()
    res = R.compare_depth(rc, got, S.DEPTH_ERROR_BOUND, 1.0)
    report(record_property, f"ur_shadow_map, shadow {w}x{h}", res)
    assert R.failures(res) == 0, res


@pytest.mark.parametrize("w,h", R.TARGETS)
@pytest.mark.parametrize("name", ["icosphere", "torus"])
def test_depth_prepass_and_gbuffer(hotpath, record_property, name, w, h):
    sc, rc = R.cast_scene(name, w, h)
    depth, got = camera_passes(hotpath, sc, sc.draws, w, h)
    held(record_property, f"ur_depth_prepass + ur_gbuffer_pass, {name} {w}x{h}", rc, sc.draws, depth, got)


@pytest.mark.parametrize("w,h", R.TARGETS)
def test_near_plane_strip_with_and_without_the_queue(hotpath, record_property, w, h):
    """The strip's cut triangles and the two target-spanning ones, through the large-triangle queue and, with no queue, through the wave
    that found them."""
    sc, rc = R.cast_scene("near-plane strip", w, h)
    try:
        for reserve in (1 << 12, 0):
            hotpath.raster_reserve(reserve)
            depth, got = camera_passes(hotpath, sc, sc.draws, w, h)
            held(record_property, f"ur_depth_prepass + ur_gbuffer_pass, near-plane strip {w}x{h}, queue of {reserve}", rc, sc.draws, depth, got)
    finally:
        hotpath.raster_reserve(0)


@pytest.mark.parametrize("w,h", R.TARGETS)
def test_two_draws_in_both_orders(hotpath, record_property, w, h):
    sc, rc = R.cast_scene("two draws", w, h)
    compared = R.classify(rc)[0]
    both = []
    for order in (1, -1):
        depth, got = camera_passes(hotpath, sc, sc.draws[::order], w, h)
        held(record_property, f"ur_depth_prepass + ur_gbuffer_pass, two draws {w}x{h}, order {order}", rc, sc.draws, depth, got)
        both.append(got)
    for k in ("A", "B", "C", "hdr", "object_id"):
        assert np.array_equal(both[0][k][compared], both[1][k][compared]), k
