"""Footprint rules (tests/footprint.py, run_rules unchanged) for ur_mesh_build: it reads the glTF buffer's bytes
alone and writes the 64 * V vertex bytes, the 4 * I index bytes, the info record and inside the layout's scratch bytes. The buffer, the
vertices, the indices, the scratch and the info record sit between guards; the write rule (hash guards) and the read rule (0xFF and zero
guards against plain tensors) hold for the soup, where both passes and the out-of-range indices run, for the two long segments, and for
the outputs placed at every 16-byte phase the header allows (vertices and scratch at 16, indices and info at 4, 8 and 16, the buffer
at 4)."""
import numpy as np
import pytest

from tests import footprint as fp
from tests import mesh_cases as M
from tests import mesh_ref as R

pytestmark = pytest.mark.gpu

POISON = 0x5A


def _guarded_build(hotpath, urlib, name, aligns=None):
    from unclerenderer_amd import hostmath, lib
    data, prims = M.case(name)
    records = M.host_primitives(prims)
    layout, _ = hostmath.mesh_layout(records, len(data))
    array = hostmath.mesh_primitive_array(records)
    V, I, scratch = layout.vertex_count, layout.index_count, int(layout.scratch_bytes)

    def call(b):
        lib.check(urlib.ur_mesh_build(hotpath.ctx, b["buffer"].data_ptr(), len(data), array, len(records), b["vertices"].data_ptr(), b["indices"].data_ptr(),
                                      b["scratch"].data_ptr(), scratch, b["info"].data_ptr()), "ur_mesh_build")

    outputs = {"vertices": np.full(64 * V, POISON, np.uint8), "indices": np.full(4 * I, POISON, np.uint8), "info": np.full(56, POISON, np.uint8)}
    # the scratch is the build's own: guarded against overruns (write rule); its content after the call is not a result, so it is an
    # output of no run (a second, plain rule over it would compare cursors the atomics filled in any order)
    guarded_scratch = {}

    def call_with_scratch(b):
        import torch
        s = fp.guarded(np.full(scratch, 0xFF, np.uint8), "cuda", ("hash", 77), (aligns or {}).get("scratch", fp.GRAIN), 64)
        guarded_scratch["last"] = s
        call({**b, "scratch": s})
        torch.cuda.synchronize()
        report = fp.check(s)
        assert report.ok, f"ur_mesh_build, {name}: write rule, scratch: {report}"

    got = fp.run_rules(call_with_scratch, {"buffer": np.frombuffer(data, np.uint8)}, outputs, aligns=aligns,
                       row_bytes={"vertices": 64, "indices": 12, "buffer": 4, "info": 56}, what=f"ur_mesh_build, {name}, aligns {aligns}")
    vertices, indices, _, info = M.expected(name)
    assert np.array_equal(got["vertices"].view(np.uint32).reshape(-1, 16), vertices)
    assert np.array_equal(got["indices"].view(np.uint32), indices)
    assert got["info"].tobytes() == R.info_bytes(info)


@pytest.mark.parametrize("name", ["soup", "fans", "modes_5121", "two_primitives", "count_1"])
def test_the_build_touches_its_own_bytes_alone(hotpath, urlib, name):
    _guarded_build(hotpath, urlib, name)


@pytest.mark.parametrize("phase", [4, 8, 16])
def test_placements_at_every_phase(hotpath, urlib, phase):
    _guarded_build(hotpath, urlib, "soup", aligns={"vertices": 16, "scratch": 16, "indices": phase, "info": phase, "buffer": 4})
