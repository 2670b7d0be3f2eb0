"""Footprint of ur_env_cube_build (include/ur_env_cube.h) by the rules of tests/footprint.py: guards around the source, the destination and the
info word stay intact, the source keeps its bytes, and the destination and the info word are the host build's whether the guards around the
source are 0xFF or zero bytes and whatever the destination held before (every byte of it is written: hashed guards with another seed per
run give it other prior bytes each time)."""
import numpy as np
import pytest

from tests import env_cube_ref as R
from tests import footprint as F

pytestmark = pytest.mark.gpu


def run(hotpath, fmt, base, mips, poison, run_index, with_info=True):
    import torch
    from unclerenderer_amd import hostmath
    payload = R.random_payload(300 + base, fmt, base, mips)
    want, bad = hostmath.env_cube_build(payload, fmt, base, mips)
    src = F.guarded(payload, "cuda", poison, 16)
    prior = np.random.default_rng(base + run_index).integers(0, 65536, want.shape, dtype=np.uint16)
    dst = F.guarded(prior, "cuda", ("hash", 2 * F.hash_seed("dst") + run_index), 16, row_bytes=8 * (base + 2))
    info = F.guarded(np.full(1, 0x7F7F7F7F, np.int32), "cuda", ("hash", 2 * F.hash_seed("info") + run_index), 4) if with_info else None
    hotpath.build_env_cube(src, fmt, base, mips, info, out=dst)
    torch.cuda.synchronize()
    for name, view in (("source", src), ("destination", dst), ("info", info)):
        if view is not None:
            r = F.check(view)
            assert r.ok, f"write rule, {name} ({poison} guards, format {fmt}, base {base}, {mips} mips): {r}"
    assert np.array_equal(F.host_bytes(src), payload), "the source was written"
    got = F.host_bytes(dst)
    assert np.array_equal(got, want.view(np.uint8).reshape(-1)), f"read rule ({poison} guards, format {fmt}, base {base}, {mips} mips)"
    if with_info:
        assert F.host_bytes(info).view(np.int32).tolist() == [bad]
    return got


@pytest.mark.parametrize("fmt,base,mips", [(R.SF16, 1, 1), (R.SF16, 5, 3), (R.UF16, 6, 1), (R.SF16, 33, 6), (R.RGBA16F, 3, 2), (R.RGBA16F, 33, 6), (R.UF16, 64, 7)])
def test_env_cube_build_footprint(hotpath, fmt, base, mips):
    ones = run(hotpath, fmt, base, mips, "ones", 0)
    zeros = run(hotpath, fmt, base, mips, "zeros", 1)
    assert np.array_equal(ones, zeros)
    none = run(hotpath, fmt, base, mips, "ones", 2, with_info=False)
    assert np.array_equal(ones, none)
