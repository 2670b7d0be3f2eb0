"""ur_env_panorama on the device (include/ur_env_panorama.h): byte-equal to ur_host_env_panorama - which
tests/test_env_panorama_ref.py holds to the numpy restatement - over seeded panoramas (subnormal texels, e = 0 and texels beyond fp16
among them), into a destination that arrives as 0xFF and as zero; the same call twice; two calls queued into one destination; the Python
function from an array, from bytes and from a device tensor; the whole route through ur_env_prefilter and ur_env_cube_build against the
host route staged by ur_stage_env_cube; and the lighting pass over the two cubes."""
import numpy as np
import pytest

from tests import env_panorama_ref as R

pytestmark = pytest.mark.gpu

# (W, H, E, K). On 67 x 33: waves that hold 64, 16 and 4 texels with a partial last wave (K = 1: E = 1 is six texels in one wave;
# K = 4: 6 E^2 / 4 waves), a texel a wave (K = 8), four taps a lane (K = 16), one workgroup and several. Then a larger cube with two
# taps a side, and the widest and the tallest panorama.
CASES = [(67, 33, e, k) for e in (1, 2, 4, 8, 16, 32) for k in (1, 4, 8, 16)] + [(256, 128, 64, 2), (16384, 1, 8, 4), (1, 8192, 8, 4)]


@pytest.fixture(scope="module")
def panoramas():
    out = {(w, h): R.random_panorama(5000 + w + h, w, h) for w, h in {c[:2] for c in CASES}}
    for a in out.values():
        a.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def host_built(urlib, panoramas):
    """{case: the host build's cube}: computed once, shared and left unchanged."""
    from unclerenderer_amd import hostmath
    out = {}
    for case in CASES:
        want = hostmath.env_panorama(panoramas[case[:2]], *case)
        want.setflags(write=False)
        out[case] = want
    return out


def device_cube(t):
    return t.cpu().numpy().view(np.uint16).reshape(6, t.shape[1], t.shape[2], 4)


@pytest.mark.parametrize("fill", [0xFF, 0x00])
def test_device_build_is_the_host_build(hotpath, panoramas, host_built, fill):
    import torch
    from unclerenderer_amd import environment
    from unclerenderer_amd.hotpath import to_device
    sources = {size: to_device(p.copy()) for size, p in panoramas.items()}
    for case, want in host_built.items():
        w, h, base, taps = case
        dst = torch.full((6, base, base, 4), -1 if fill else 0, dtype=torch.int16, device=sources[(w, h)].device)
        got = environment.panorama_to_cube(hotpath, sources[(w, h)], w, h, base, taps, out=dst)
        assert got is dst
        torch.cuda.synchronize()
        same = device_cube(dst) == want
        assert same.all(), f"{case}, fill {fill:#x}: {np.count_nonzero(~same)} values differ, first at {tuple(np.argwhere(~same)[0])}"
    for size, p in panoramas.items():
        assert np.array_equal(sources[size].cpu().numpy(), p)  # the inputs are as they were


def test_same_call_twice_from_an_array_bytes_and_a_tensor(hotpath, panoramas, host_built):
    """The function allocates the destination itself and takes the recommended taps; an array, bytes and a device tensor give the same
    bytes, the host's."""
    import torch
    from unclerenderer_amd import environment, hostmath
    from unclerenderer_amd.hotpath import to_device
    pano = panoramas[(67, 33)]
    assert hostmath.env_panorama_taps(67, 33, 16) == 4
    want = host_built[(67, 33, 16, 4)]
    a = environment.panorama_to_cube(hotpath, pano, 67, 33, 16)
    b = environment.panorama_to_cube(hotpath, pano.tobytes(), 67, 33, 16)
    c = environment.panorama_to_cube(hotpath, to_device(pano.copy()), 67, 33, 16, 4)
    d = environment.panorama_to_cube(hotpath, pano, 67, 33, 16)
    torch.cuda.synchronize()
    for got in (a, b, c, d):
        assert got.shape == (6, 16, 16, 4) and got.dtype == torch.int16 and np.array_equal(device_cube(got), want)


def test_two_calls_queued_into_one_destination(hotpath, panoramas, host_built):
    """Two different panoramas of one size, built back to back into the same destination with nothing between them: the second one's bytes."""
    import torch
    from unclerenderer_amd import environment, hostmath
    from unclerenderer_amd.hotpath import to_device
    case = (67, 33, 32, 4)
    other = R.random_panorama(77, 67, 33)
    want_b = hostmath.env_panorama(other, *case)
    assert not np.array_equal(host_built[case], want_b)
    a, b = to_device(panoramas[(67, 33)].copy()), to_device(other)
    dst = torch.empty((6, 32, 32, 4), dtype=torch.int16, device=a.device)
    environment.panorama_to_cube(hotpath, a, *case, out=dst)
    environment.panorama_to_cube(hotpath, b, *case, out=dst)
    torch.cuda.synchronize()
    assert np.array_equal(device_cube(dst), want_b)


@pytest.fixture(scope="module")
def routes(hotpath):
    """{E: (the cube baked on the device from the panorama, the host route - hostmath.env_panorama, hostmath.env_prefilter - staged by
    ur_stage_env_cube)} at 64 samples, from a smooth 128 x 64 panorama with a sun beyond fp16."""
    import torch
    from unclerenderer_amd import environment, hostmath
    pano = R.to_rgbe(R.environment(3)(R.panorama_directions(128, 64))).copy()
    pano[20:22, 90:92] = (255, 240, 200, 150)  # 255 * 2^14: the clamp keeps the prefilter's contract
    out = {}
    for base in (16, 32):
        top = hostmath.env_panorama(pano, 128, 64, base)
        assert (top[..., :3] == 0x7BFF).any() and (top[..., :3] < 0x7C00).all()
        payload = hostmath.env_prefilter(top, base, 64)
        baked = environment.bake_panorama(hotpath, pano, 128, 64, base, 64)
        staged = hotpath.stage_env_cube(payload, base, base.bit_length())
        torch.cuda.synchronize()
        out[base] = (baked, staged)
    return out


@pytest.mark.parametrize("base", [16, 32])
def test_bake_panorama_is_the_staged_host_route(routes, base):
    import torch
    baked, staged = routes[base]
    assert baked.shape == staged.shape and baked.dtype == staged.dtype and torch.equal(baked, staged)


@pytest.mark.parametrize("w,h", [(64, 64), (50, 40)])
def test_lighting_over_a_baked_panorama(hotpath, routes, w, h):
    """ur_deferred_lighting at 64 x 64 (the streaming kernel) and 50 x 40 (the per-tile kernel): over the cube baked on the device from the
    panorama the result is byte-equal to the same call over the host route's cube staged by ur_stage_env_cube."""
    import torch
    from tests.test_gpu_parity import _lighting_inputs
    from unclerenderer_amd.hotpath import to_device
    fc, g, shadow, _, lut = _lighting_inputs("sponza", w, h, seed=21, mode="scene")
    d_shadow, d_lut = to_device(shadow), to_device(lut)
    dA, dB, dC = to_device(g.A), to_device(g.B), to_device(g.C)
    out = []
    for cube in routes[32]:
        hdr = to_device(g.hdr)
        hotpath.deferred_lighting(fc.scene, dA, dB, dC, hotpath.make_tables(d_shadow, cube, 32, 6, d_lut), hdr, w, h)
        torch.cuda.synchronize()
        out.append(hdr.cpu().numpy().view(np.uint16))
    assert np.array_equal(out[0], out[1])
    assert not np.array_equal(out[0], g.hdr.view(np.uint16))  # the pass wrote something
