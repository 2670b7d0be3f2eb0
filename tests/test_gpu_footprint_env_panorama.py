"""Footprint of ur_env_panorama (include/ur_env_panorama.h) by the rules of tests/footprint.py: guards around the source and the
destination stay intact, the source keeps its bytes, and the destination is the host build's whether the guards are 0xFF or zero bytes
and whatever the destination held before (every byte of it is written). The buffers are of exactly the sizes the header names and at the
weakest alignments it allows - the source 4-byte, the destination 16-byte aligned - so a stray access lands in a guard."""
import numpy as np
import pytest

from tests import env_panorama_ref as R
from tests import footprint as F

pytestmark = pytest.mark.gpu

W, H = 67, 33


def run(hotpath, base, taps, poison, run_index):
    import torch
    from unclerenderer_amd import environment, hostmath
    pano = R.random_panorama(400 + base + taps, W, H)
    want = hostmath.env_panorama(pano, W, H, base, taps)
    src = F.guarded(pano.reshape(-1, 4), "cuda", poison, 4)
    rng = np.random.default_rng(base + run_index)
    dst = F.guarded(rng.integers(0, 65536, (6 * base * base, 4), dtype=np.uint16), "cuda", poison, 16)
    environment.panorama_to_cube(hotpath, src, W, H, base, taps, out=dst)
    torch.cuda.synchronize()
    for name, view in (("source", src), ("destination", dst)):
        r = F.check(view)
        assert r.ok, f"write rule, {name} ({poison} guards, base {base}, {taps} taps): {r}"
    assert np.array_equal(F.host_bytes(src), pano.reshape(-1)), "the source was written"
    got = F.host_bytes(dst)
    assert np.array_equal(got, want.view(np.uint8).reshape(-1)), f"read rule ({poison} guards, base {base}, {taps} taps)"
    return got


@pytest.mark.parametrize("base", [1, 4, 32])
@pytest.mark.parametrize("taps", [1, 8])
def test_env_panorama_footprint(hotpath, base, taps):
    ones = run(hotpath, base, taps, "ones", 0)
    zeros = run(hotpath, base, taps, "zeros", 1)
    assert np.array_equal(ones, zeros)
