"""Footprints of ur_env_sky and ur_brdf_lut (include/ur_env_sky.h, include/ur_brdf_lut.h) by the rules of tests/footprint.py: guards
around the destination of the capture, and around the table and the destination of the LUT, stay intact (the write rule); the table keeps
its bytes; and the destinations are the host builds' whether the guards are 0xFF or zero bytes and whatever the destinations held before
(the read rule: every byte is written, nothing outside the named bytes is read into the result). The buffers are of exactly the sizes the
headers name and at the weakest alignment they allow, 16 bytes, so a stray access lands in a guard."""
import numpy as np
import pytest

from tests import env_sky_ref as R
from tests import footprint as F

pytestmark = pytest.mark.gpu


def run_sky(hotpath, base, taps, poison, run_index):
    import torch
    from unclerenderer_amd import environment, hostmath
    sky = R.sky_constants((0.3, 0.8, -0.5))
    want = hostmath.env_sky(sky, base, taps)
    rng = np.random.default_rng(base + run_index)
    dst = F.guarded(rng.integers(0, 65536, (6 * base * base, 4), dtype=np.uint16), "cuda", poison, 16)
    environment.sky_to_cube(hotpath, sky, base, taps, out=dst)
    torch.cuda.synchronize()
    r = F.check(dst)
    assert r.ok, f"write rule, destination ({poison} guards, base {base}, {taps} taps): {r}"
    got = F.host_bytes(dst)
    assert np.array_equal(got, want.view(np.uint8).reshape(-1)), f"read rule ({poison} guards, base {base}, {taps} taps)"
    return got


@pytest.mark.parametrize("base", [1, 4, 32])
@pytest.mark.parametrize("taps", [1, 2, 8])
def test_env_sky_footprint(hotpath, base, taps):
    ones = run_sky(hotpath, base, taps, "ones", 0)
    zeros = run_sky(hotpath, base, taps, "zeros", 1)
    assert np.array_equal(ones, zeros)


def run_lut(hotpath, w, h, samples, poison, run_index):
    import torch
    from unclerenderer_amd import hostmath, lib
    from unclerenderer_amd.hotpath.tensors import _ptr, nbytes
    table = hostmath.brdf_lut_table(h, samples)
    want = hostmath.brdf_lut(w, h, samples, table=table)
    src = F.guarded(table.copy().reshape(-1, 16), "cuda", poison, 16)
    rng = np.random.default_rng(w + h + run_index)
    dst = F.guarded(rng.integers(0, 65536, (w * h, 2), dtype=np.uint16), "cuda", poison, 16)
    lib.check(hotpath._L.ur_brdf_lut(hotpath._ctx, w, h, samples, _ptr(src), nbytes(src), _ptr(dst), nbytes(dst)), "ur_brdf_lut")
    torch.cuda.synchronize()
    for name, view in (("table", src), ("destination", dst)):
        r = F.check(view)
        assert r.ok, f"write rule, {name} ({poison} guards, {w} x {h}, {samples} samples): {r}"
    assert np.array_equal(F.host_bytes(src), table.reshape(-1)), "the table was written"
    got = F.host_bytes(dst)
    assert np.array_equal(got, want.view(np.uint8).reshape(-1)), f"read rule ({poison} guards, {w} x {h}, {samples} samples)"
    return got


@pytest.mark.parametrize("w,h,samples", [(1, 1, 16), (7, 5, 64), (64, 8, 128)])
def test_brdf_lut_footprint(hotpath, w, h, samples):
    ones = run_lut(hotpath, w, h, samples, "ones", 0)
    zeros = run_lut(hotpath, w, h, samples, "zeros", 1)
    assert np.array_equal(ones, zeros)
