"""Footprint of ur_scene_build (include/ur_scene_build.h) by the rules of tests/footprint.py: guards around every table, every output and the
scratch stay intact; the bytes between 608 and the stride, the slots no draw names and (transforms only) everything but World keep what
they held; and the outputs are the restatement's whether the guards around the inputs are 0xFF or zero bytes. The commands carry the
constants' address, which differs between two allocations, so the runs are compared with the restatement at their own address and with
each other in every other byte."""
import numpy as np
import pytest

from tests import footprint as F
from tests import scene_build_ref as R
from tests.test_scene_build_ref import differing, frame, prior, same_bytes

pytestmark = pytest.mark.gpu


def run(hotpath, D, stride, poison, run_index, transforms_only=False, align=16):
    import torch
    from unclerenderer_amd import lib
    from unclerenderer_amd.hotpath import BuiltScene, SceneTables
    nodes, meshes, infos, materials, draws, slots = R.seeded_tables(300 + D, D)
    tables = {"nodes": nodes, "meshes": meshes, "mesh_infos": infos, "materials": materials, "draws": draws}
    inputs = {k: F.guarded(v.view(np.uint8).reshape(-1), "cuda", poison, align) for k, v in tables.items()}
    init = prior(np.random.default_rng(D), D, slots, stride)
    need = int(lib.load().ur_scene_build_scratch_bytes(D))
    init["scratch"] = np.random.default_rng(D + 1).integers(0, 256, need, dtype=np.uint8)
    outputs = {k: F.guarded(v, "cuda", ("hash", 2 * F.hash_seed(k) + run_index), align, row_bytes=stride if k == "constants" else None) for k, v in init.items()}
    dev = SceneTables(inputs["nodes"], inputs["meshes"], inputs["mesh_infos"], inputs["materials"], inputs["draws"], slot_count=slots, constants_stride=stride)
    built = BuiltScene(outputs["bounds"], outputs["commands"], outputs["constants"], outputs["centers"], outputs["summary"].view(torch.int32), outputs["scratch"])
    hotpath.build_scene(dev, frame(), transforms_only=transforms_only, out=built)
    torch.cuda.synchronize()
    for k, v in {**inputs, **outputs}.items():
        r = F.check(v)
        assert r.ok, f"write rule, {k} ({poison} guards, D = {D}, stride {stride}): {r}"
    for k, v in tables.items():
        assert np.array_equal(F.host_bytes(inputs[k]), v.view(np.uint8).reshape(-1)), f"input {k} was written"
    got = {k: F.host_bytes(outputs[k]).view(init[k].dtype).reshape(init[k].shape) for k in init if k != "scratch"}
    address = outputs["constants"].data_ptr()
    del init["scratch"]
    want = R.build(nodes, meshes, infos, materials, draws, frame(), slots, stride, address, out=init, transforms_only=transforms_only)
    assert same_bytes(want, got), differing(want, got)
    assert np.array_equal(got["constants"][:, 608:], init["constants"][:, 608:])
    return got, address, draws, slots


@pytest.mark.parametrize("D,stride", [(1, 608), (63, 768), (65, 608), (257, 768), (4097, 624)])
def test_scene_build_footprint(hotpath, D, stride):
    ones, address_ones, draws, slots = run(hotpath, D, stride, "ones", 0)
    zeros, address_zeros, _, _ = run(hotpath, D, stride, "zeros", 1)
    for k in ("bounds", "constants", "centers", "summary"):
        assert np.array_equal(ones[k].view(np.uint8), zeros[k].view(np.uint8)), f"read rule: {k} differs between 0xFF and zero guards"
    other = np.ones(16, bool)
    other[[8, 9]] = False
    assert np.array_equal(ones["commands"][:, other], zeros["commands"][:, other])
    live = (draws["node"] < max(1, D // 3)) & (draws["mesh"] < 5) & (draws["material"] < 7) & (draws["constants_slot"] < slots)
    at = lambda c: c[:, 8].astype(np.uint64) | (c[:, 9].astype(np.uint64) << np.uint64(32))  # noqa: E731
    assert np.array_equal((at(ones["commands"]) - np.uint64(address_ones))[live], (at(zeros["commands"]) - np.uint64(address_zeros))[live])


@pytest.mark.parametrize("D,stride", [(65, 608), (4097, 768)])
def test_transforms_only_footprint(hotpath, D, stride):
    """Commands and the bytes 64 .. stride of every record keep the prior bytes (the restatement's `out`), under both guards."""
    ones, _, _, _ = run(hotpath, D, stride, "ones", 0, transforms_only=True)
    zeros, _, _, _ = run(hotpath, D, stride, "zeros", 1, transforms_only=True)
    for k in ones:
        assert np.array_equal(ones[k].view(np.uint8), zeros[k].view(np.uint8)), k
    init = prior(np.random.default_rng(D), D, ones["constants"].shape[0], stride)
    assert np.array_equal(ones["commands"], init["commands"]) and np.array_equal(ones["constants"][:, 64:], init["constants"][:, 64:])
