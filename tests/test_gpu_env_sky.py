"""ur_env_sky on the device (include/ur_env_sky.h): byte-equal to ur_host_env_sky - which tests/test_env_sky_ref.py
holds to the numpy restatement - into a destination that arrives as 0xFF and as zero; the same call twice; two suns queued into one
destination; the closed loop - every face of the capture against ur_sky_atmosphere rendered through a camera that looks along that
face -; the whole route through ur_env_prefilter and ur_env_cube_build against the host route staged by ur_stage_env_cube; and the
lighting pass over the two cubes, and under a sun that moved."""
import numpy as np
import pytest

from tests import env_sky_ref as R

pytestmark = pytest.mark.gpu

# (E, K): waves that hold 64, 4 texels and one, with a partial last wave (E = 1: six texels in one wave), four taps a lane (K = 16), one
# workgroup and several; then a larger cube with two taps a side (16 texels a wave).
CASES = [(e, k) for e in (1, 2, 4, 8, 16, 32) for k in (1, 4, 16)] + [(64, 2)]
SUN, OTHER_SUN = (0.3, 0.8, -0.5), (-0.7, 0.25, 0.4)


@pytest.fixture(scope="module")
def host_built(urlib):
    """{case: the host build's cube}: computed once, shared and left unchanged."""
    from unclerenderer_amd import hostmath
    out = {}
    for case in CASES:
        want = hostmath.env_sky(R.sky_constants(SUN), *case)
        want.setflags(write=False)
        out[case] = want
    return out


def device_cube(t):
    return t.cpu().numpy().view(np.uint16).reshape(6, t.shape[1], t.shape[2], 4)


@pytest.mark.parametrize("fill", [0xFF, 0x00])
def test_device_capture_is_the_host_capture(hotpath, host_built, fill):
    import torch
    from unclerenderer_amd import environment
    sky = R.sky_constants(SUN)
    for case, want in host_built.items():
        base, taps = case
        dst = torch.full((6, base, base, 4), -1 if fill else 0, dtype=torch.int16, device="cuda")
        got = environment.sky_to_cube(hotpath, sky, base, taps, out=dst)
        assert got is dst
        torch.cuda.synchronize()
        same = device_cube(dst) == want
        assert same.all(), f"{case}, fill {fill:#x}: {np.count_nonzero(~same)} values differ, first at {tuple(np.argwhere(~same)[0])}"


def test_same_call_twice_and_two_suns_queued_into_one_destination(hotpath, host_built):
    import torch
    from unclerenderer_amd import environment, hostmath
    a = environment.sky_to_cube(hotpath, R.sky_constants(SUN), 16)
    b = environment.sky_to_cube(hotpath, R.sky_constants(SUN), 16, 1)
    torch.cuda.synchronize()
    for got in (a, b):
        assert got.shape == (6, 16, 16, 4) and got.dtype == torch.int16 and np.array_equal(device_cube(got), host_built[(16, 1)])
    # the constants are read before the call returns: two captures back to back into one destination leave the second one's bytes
    want = hostmath.env_sky(R.sky_constants(OTHER_SUN), 32, 4)
    assert not np.array_equal(want, host_built[(32, 4)])
    dst = torch.empty((6, 32, 32, 4), dtype=torch.int16, device="cuda")
    sky = R.sky_constants(SUN)
    environment.sky_to_cube(hotpath, sky, 32, 4, out=dst)
    sky.LightDirection[:] = list(OTHER_SUN)
    environment.sky_to_cube(hotpath, sky, 32, 4, out=dst)
    torch.cuda.synchronize()
    assert np.array_equal(device_cube(dst), want)


def face_camera(face, sun):
    """The sky constants of a camera with a 90-degree square frustum that looks along `face`: its right and down axes are the face
    table's d/ds and d/dt, so pixel (x, y) of an E x E frame looks through texel (x, y) of the face."""
    sky = R.sky_constants(sun)
    forward, right, down = (np.array(R.FACES[face](s, t, o), np.float32) for s, t, o in ((0.0, 0.0, 1.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)))
    view = np.zeros((4, 4), np.float32)
    view[:3, 0], view[:3, 1], view[:3, 2], view[3, 3] = right, -down, forward, 1.0  # world = vx right + vy up + forward
    proj = np.zeros(16, np.float32)
    proj[0], proj[5], proj[11], proj[14] = 1.0, 1.0, 1.0, 0.1  # reverse-Z infinite, near 0.1
    world = np.zeros(16, np.float32)
    world[0], world[5], world[10], world[15] = 100.0, 100.0, 100.0, 1.0
    sky.View[:], sky.Projection[:], sky.World[:] = view.reshape(-1).tolist(), proj.tolist(), world.tolist()
    return sky


@pytest.mark.parametrize("E", [16, 64])
def test_the_capture_is_the_sky_the_frame_draws(hotpath, E):
    """The closed loop: for each face, ur_sky_atmosphere at E x E over cleared depth through that face's camera against the face of the
    one-tap capture. Each side is within max(1e-3, one fp16 ulp) of the float64 shader, so they differ by at most twice that. A capture
    whose +Y and -Y faces are exchanged does not pass."""
    import torch
    from unclerenderer_amd import environment
    capture = R.cube_of(device_cube(environment.sky_to_cube(hotpath, R.sky_constants(SUN), E, 1)))
    depth = torch.zeros((E, E), dtype=torch.float32, device="cuda")
    frames = []
    for face in range(6):
        hdr = torch.zeros((E, E, 4), dtype=torch.int16, device="cuda")
        hotpath.sky_atmosphere(face_camera(face, SUN), depth, hdr, E, E)
        torch.cuda.synchronize()
        frame = hdr.cpu().numpy().view(np.float16).astype(np.float64)
        assert (frame[..., 3] == 1.0).all()  # the sky covered every pixel
        frames.append(frame[..., :3])
    frames = np.stack(frames)
    bound = 2 * np.maximum(1e-3, R.half_ulp(frames))
    excess = np.abs(frames - capture) - bound
    print(f"E {E}: largest difference {np.abs(frames - capture).max():.6f}")
    assert (excess <= 0).all(), f"E {E}: {np.count_nonzero(excess > 0)} values beyond twice max(1e-3, 1 fp16 ulp), worst excess {excess.max()}"
    exchanged = capture[[0, 1, 3, 2, 4, 5]]
    assert (np.abs(frames - exchanged) > bound).any()


@pytest.fixture(scope="module")
def routes(hotpath):
    """{E: (the cube baked on the device from the sky, the host route - hostmath.env_sky, hostmath.env_prefilter - staged by
    ur_stage_env_cube, the cube baked under another sun)} at 64 samples."""
    import torch
    from unclerenderer_amd import environment, hostmath
    out = {}
    for base in (16, 32):
        payload = hostmath.env_prefilter(hostmath.env_sky(R.sky_constants(SUN), base, 1), base, 64)
        baked = environment.bake_sky(hotpath, R.sky_constants(SUN), base, 64)
        moved = environment.bake_sky(hotpath, R.sky_constants(OTHER_SUN), base, 64)
        staged = hotpath.stage_env_cube(payload, base, base.bit_length())
        torch.cuda.synchronize()
        out[base] = (baked, staged, moved)
    return out


@pytest.mark.parametrize("base", [16, 32])
def test_bake_sky_is_the_staged_host_route(routes, base):
    import torch
    baked, staged, moved = routes[base]
    assert baked.shape == staged.shape and baked.dtype == staged.dtype and torch.equal(baked, staged)
    assert not torch.equal(baked, moved)


@pytest.mark.parametrize("w,h", [(64, 64), (50, 40)])
def test_lighting_over_a_baked_sky(hotpath, routes, w, h):
    """ur_deferred_lighting at 64 x 64 (the streaming kernel) and 50 x 40 (the per-tile kernel): over the cube baked on the device from the
    sky the result is byte-equal to the same call over the host route's cube; over the cube of a sun that moved it is another."""
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
    assert not np.array_equal(out[0], out[2])  # moving the sun changes the lit image
