"""ur_brdf_lut on the device (include/ur_brdf_lut.h): byte-equal to ur_host_brdf_lut - which tests/test_brdf_lut_ref.py
holds to the numpy restatement - into a destination that arrives as 0xFF and as zero; a second call queued behind the first; and the
lighting pass over the device-made and the host-made table."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# one texel; fewer texels than a workgroup's four waves; odd sizes with a partial last workgroup; many workgroups; the lighting's size.
# 16 samples leave 48 lanes idle, 64 give a lane one sample, 1024 sixteen.
CASES = [(w, h, s) for w, h in ((1, 1), (3, 2), (7, 5), (64, 8)) for s in (16, 64)] + [(128, 32, 1024)]


@pytest.fixture(scope="module")
def host_built(urlib):
    """{case: the host build's table}: computed once, shared and left unchanged."""
    from unclerenderer_amd import hostmath
    out = {}
    for case in CASES:
        want = hostmath.brdf_lut(*case)
        want.setflags(write=False)
        out[case] = want
    return out


def device_lut(t):
    return t.cpu().numpy().view(np.uint16).reshape(t.shape)


@pytest.mark.parametrize("fill", [0xFF, 0x00])
def test_device_table_is_the_host_table(hotpath, host_built, fill):
    import torch
    from unclerenderer_amd import environment
    for case, want in host_built.items():
        w, h, s = case
        dst = torch.full((h, w, 2), -1 if fill else 0, dtype=torch.int16, device="cuda")
        got = environment.brdf_lut(hotpath, w, h, s, out=dst)
        assert got is dst
        torch.cuda.synchronize()
        same = device_lut(dst) == want
        assert same.all(), f"{case}, fill {fill:#x}: {np.count_nonzero(~same)} values differ, first at {tuple(np.argwhere(~same)[0])}"


def test_a_second_call_queued_behind_the_first(hotpath, host_built):
    """The function allocates the destination itself; two builds with different sample counts back to back into one destination leave
    the second one's bytes."""
    import torch
    from unclerenderer_amd import environment
    a = environment.brdf_lut(hotpath, 64, 8, 64)
    torch.cuda.synchronize()
    assert a.shape == (8, 64, 2) and a.dtype == torch.uint16 and np.array_equal(device_lut(a), host_built[(64, 8, 64)])
    assert not np.array_equal(host_built[(64, 8, 16)], host_built[(64, 8, 64)])
    dst = torch.empty((8, 64, 2), dtype=torch.uint16, device="cuda")
    environment.brdf_lut(hotpath, 64, 8, 16, out=dst)
    environment.brdf_lut(hotpath, 64, 8, 64, out=dst)
    torch.cuda.synchronize()
    assert np.array_equal(device_lut(dst), host_built[(64, 8, 64)])


@pytest.mark.parametrize("w,h", [(64, 64), (50, 40)])
def test_lighting_over_a_device_made_table(hotpath, host_built, w, h):
    """ur_deferred_lighting at 64 x 64 (the streaming kernel, which requires the 128 x 32 table) and 50 x 40 (the per-tile kernel): over the
    table made on the device the result is byte-equal to the same call over the host-made table uploaded; and not what another table gives."""
    import torch
    from tests.test_gpu_parity import _lighting_inputs
    from unclerenderer_amd import environment
    from unclerenderer_amd.hotpath import to_device
    fc, g, shadow, env, other = _lighting_inputs("sponza", w, h, seed=22, mode="scene")
    d_shadow, d_env = to_device(shadow), hotpath.stage_env_cube(env, 32, 6)
    dA, dB, dC = to_device(g.A), to_device(g.B), to_device(g.C)
    made = environment.brdf_lut(hotpath, 128, 32, 1024)
    out = []
    for lut in (made, to_device(host_built[(128, 32, 1024)].copy()), to_device(other)):
        hdr = to_device(g.hdr)
        hotpath.deferred_lighting(fc.scene, dA, dB, dC, hotpath.make_tables(d_shadow, d_env, 32, 6, lut), hdr, w, h)
        torch.cuda.synchronize()
        out.append(hdr.cpu().numpy().view(np.uint16))
    assert np.array_equal(out[0], out[1])
    assert not np.array_equal(out[0], g.hdr.view(np.uint16)) and not np.array_equal(out[0], out[2])
