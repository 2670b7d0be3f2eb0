"""ur_env_prefilter on the device (include/ur_env_prefilter.h): byte-equal to ur_host_env_prefilter - which
tests/test_env_prefilter_ref.py holds to the numpy restatement - over seeded finite cubes, into a destination and a scratch that arrive as
0xFF and as zero; two calls queued into one destination; the same call twice; the whole route through ur_env_cube_build against the
host-built payload staged by ur_stage_env_cube; and the lighting pass over the two cubes."""
import numpy as np
import pytest

from tests import env_prefilter_ref as P

pytestmark = pytest.mark.gpu

# (base, samples): every base up to 32 with fewer samples than lanes and with as many, a level of more than one filter group of several
# workgroups (64, 256), and the largest table a workgroup can hold, 64 KiB of LDS (4, 4096)
CASES = [(b, s) for b in (1, 2, 4, 8, 16, 32) for s in (16, 64)] + [(64, 256), (4, 4096)]


@pytest.fixture(scope="module")
def host_built(urlib):
    """{(base, samples): (top level, table, the host build's payload)}: computed once, shared and left unchanged."""
    from unclerenderer_amd import hostmath
    out = {}
    for base, samples in CASES:
        top = P.random_cube(9000 + 10 * base + samples, base)
        table = hostmath.env_prefilter_table(base, samples)
        want = hostmath.env_prefilter(top, base, samples, table=table)
        for a in (top, table, want):
            a.setflags(write=False)
        out[(base, samples)] = (top, table, want)
    return out


def device_bytes(t):
    return t.cpu().numpy().view(np.uint16).reshape(-1, 4)


@pytest.mark.parametrize("fill", [0xFF, 0x00])
def test_device_prefilter_is_the_host_prefilter(hotpath, urlib, host_built, fill):
    import torch
    from unclerenderer_amd.hotpath import to_device
    for (base, samples), (top, table, want) in host_built.items():
        src, tab = to_device(top.copy()), to_device(table.copy())
        dst = torch.full((want.shape[0], 4), -1 if fill else 0, dtype=torch.int16, device=src.device)
        scratch = torch.full((int(urlib.ur_env_prefilter_scratch_bytes(base)),), fill, dtype=torch.uint8, device=src.device)
        got = hotpath.prefilter_env_cube(src, base, samples, table=tab, out=dst, scratch=scratch)
        assert got is dst
        torch.cuda.synchronize()
        same = device_bytes(dst).view(np.uint8) == want.view(np.uint8)
        assert same.all(), f"base {base}, {samples} samples, fill {fill:#x}: {np.count_nonzero(~same)} bytes differ, first at {int(np.flatnonzero(~same.reshape(-1))[0])}"
        assert np.array_equal(src.cpu().numpy().view(np.uint16), top.view(np.uint16)) and np.array_equal(tab.cpu().numpy(), table)  # the inputs are as they were


def test_same_call_twice_and_the_wrapper_s_own_buffers(hotpath, host_built):
    """The wrapper makes the table and allocates destination and scratch itself; two runs give the same bytes, the host's."""
    import torch
    for key in ((32, 64), (8, 16)):
        top, _, want = host_built[key]
        a = hotpath.prefilter_env_cube(top, *key)
        b = hotpath.prefilter_env_cube(top.tobytes(), *key)
        torch.cuda.synchronize()
        assert np.array_equal(device_bytes(a), want) and np.array_equal(device_bytes(b), want)


def test_two_calls_queued_into_one_destination(hotpath, urlib, host_built):
    """Two different cubes of one shape, filtered back to back into the same destination and scratch with nothing between them: the second
    one's bytes."""
    import torch
    from unclerenderer_amd import hostmath
    from unclerenderer_amd.hotpath import to_device
    base, samples = 32, 64
    top_a, table, want_a = host_built[(base, samples)]
    top_b = P.random_cube(77, base)
    want_b = hostmath.env_prefilter(top_b, base, samples, table=table)
    assert not np.array_equal(want_a, want_b)
    a, b, tab = to_device(top_a.copy()), to_device(top_b), to_device(table.copy())
    dst = torch.empty((want_a.shape[0], 4), dtype=torch.int16, device=a.device)
    scratch = torch.empty(int(urlib.ur_env_prefilter_scratch_bytes(base)), dtype=torch.uint8, device=a.device)
    hotpath.prefilter_env_cube(a, base, samples, table=tab, out=dst, scratch=scratch)
    hotpath.prefilter_env_cube(b, base, samples, table=tab, out=dst, scratch=scratch)
    torch.cuda.synchronize()
    assert np.array_equal(device_bytes(dst), want_b)


@pytest.fixture(scope="module")
def route(hotpath):
    """The 32-edge environment of the lighting tests, its top level alone: (the cube baked on the device, the host-built payload staged by
    ur_stage_env_cube), both staged cubes of 6 mips."""
    import torch
    from tests.test_gpu_parity import _lighting_inputs
    from unclerenderer_amd import hostmath
    env = np.ascontiguousarray(_lighting_inputs("sponza", 64, 64, seed=21, mode="scene")[3], np.uint16)
    top = P.level_of_payload(env, 32, 0)
    payload = hostmath.env_prefilter(top, 32, 64)
    baked = hotpath.bake_env_cube(top, 32, 64)
    staged = hotpath.stage_env_cube(payload, 32, 6)
    torch.cuda.synchronize()
    assert not np.array_equal(payload, env)  # (the filtered chain is not the procedural one)
    return baked, staged


def test_bake_env_cube_is_the_staged_host_payload(route):
    import torch
    baked, staged = route
    assert baked.shape == staged.shape and baked.dtype == staged.dtype and torch.equal(baked, staged)


@pytest.mark.parametrize("w,h", [(64, 64), (50, 40)])
def test_lighting_over_a_baked_cube(hotpath, route, w, h):
    """ur_deferred_lighting at 64 x 64 (the streaming kernel) and 50 x 40 (the per-tile kernel): over the cube baked on the device the
    result is byte-equal to the same call over the host-built payload staged by ur_stage_env_cube."""
    import torch
    from tests.test_gpu_parity import _lighting_inputs
    from unclerenderer_amd.hotpath import to_device
    fc, g, shadow, _, lut = _lighting_inputs("sponza", w, h, seed=21, mode="scene")
    d_shadow, d_lut = to_device(shadow), to_device(lut)
    dA, dB, dC = to_device(g.A), to_device(g.B), to_device(g.C)
    out = []
    for cube in route:
        hdr = to_device(g.hdr)
        hotpath.deferred_lighting(fc.scene, dA, dB, dC, hotpath.make_tables(d_shadow, cube, 32, 6, d_lut), hdr, w, h)
        torch.cuda.synchronize()
        out.append(hdr.cpu().numpy().view(np.uint16))
    assert np.array_equal(out[0], out[1])
    assert not np.array_equal(out[0], g.hdr.view(np.uint16))  # the pass wrote something
