"""Footprint of ur_env_prefilter (include/ur_env_prefilter.h) by the rules of tests/footprint.py: guards around the source, the table, the
scratch and the destination stay intact, the source and the table keep their bytes, and the destination is the host build's whether the
guards around the inputs are 0xFF or zero bytes and whatever destination and scratch held before (every byte of the destination is
written; the scratch is written before it is read: hashed guards with another seed per run give both other prior bytes each time). The
buffers are of exactly the sizes the header names, so a stray access lands in a guard."""
import numpy as np
import pytest

from tests import env_prefilter_ref as P
from tests import footprint as F

pytestmark = pytest.mark.gpu


def run(hotpath, urlib, base, samples, poison, run_index):
    import torch
    from unclerenderer_amd import hostmath
    top = P.random_cube(400 + base + samples, base)
    table = hostmath.env_prefilter_table(base, samples)
    want = hostmath.env_prefilter(top, base, samples, table=table)
    src = F.guarded(top.reshape(-1, 4), "cuda", poison, 16)
    tab = F.guarded(table, "cuda", poison, 16)
    rng = np.random.default_rng(base + run_index)
    dst = F.guarded(rng.integers(0, 65536, want.shape, dtype=np.uint16), "cuda", ("hash", 2 * F.hash_seed("dst") + run_index), 16)
    scratch = F.guarded(rng.integers(0, 256, int(urlib.ur_env_prefilter_scratch_bytes(base)), dtype=np.uint8), "cuda",
                        ("hash", 2 * F.hash_seed("scratch") + run_index), 16)
    hotpath.prefilter_env_cube(src, base, samples, table=tab, out=dst, scratch=scratch)
    torch.cuda.synchronize()
    for name, view in (("source", src), ("table", tab), ("destination", dst), ("scratch", scratch)):
        r = F.check(view)
        assert r.ok, f"write rule, {name} ({poison} guards, base {base}, {samples} samples): {r}"
    assert np.array_equal(F.host_bytes(src), top.view(np.uint8).reshape(-1)), "the source was written"
    assert np.array_equal(F.host_bytes(tab), table), "the table was written"
    got = F.host_bytes(dst)
    assert np.array_equal(got, want.view(np.uint8).reshape(-1)), f"read rule ({poison} guards, base {base}, {samples} samples)"
    return got


@pytest.mark.parametrize("base,samples", [(1, 16), (2, 16), (4, 64), (16, 32), (32, 64), (64, 128)])
def test_env_prefilter_footprint(hotpath, urlib, base, samples):
    ones = run(hotpath, urlib, base, samples, "ones", 0)
    zeros = run(hotpath, urlib, base, samples, "zeros", 1)
    assert np.array_equal(ones, zeros)
